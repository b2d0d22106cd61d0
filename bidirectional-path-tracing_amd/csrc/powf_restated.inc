// glibc 2.35 powf (sysdeps/ieee754/flt-32/e_powf.c, !TOINT_INTRINSICS), restated
// bit for bit. Included textually by device_math.hpp (the kernels' glibc_powf)
// and by scene.cpp (the host's gamma expansion of bitmap texels), so both sides
// run the same source. The includer defines, before the #include:
//   BDPT_PF_TABLE     storage of the two tables (static __constant__ / static const)
//   BDPT_PF_INLINE    attributes of the small helpers
//   BDPT_PF_NOINLINE  attributes of the special-case path
//   BDPT_PF_ENTRY     attributes of glibc_powf itself
// and the bit casts f2u(float), pf_u2f(uint32_t), d_from_u(uint64_t), u_from_d(double).

// glibc __powf_log2_data (POWF_LOG2_TABLE_BITS = 4): {invc, logc}
BDPT_PF_TABLE double kPowfLog2Tab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010b0p+0, -0x1.7418b0a1fb77bp-2}, {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8ea0p+0, -0x1.97c1d1b3b7af0p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aa0p-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}};

// glibc __exp2f_data (EXP2F_TABLE_BITS = 5).
BDPT_PF_TABLE uint64_t kExp2fTab[32] = {
    0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51, 0x3fef72b83c7d517b,
    0x3fef54873168b9aa, 0x3fef387a6e756238, 0x3fef1e9df51fdee1, 0x3fef06fe0a31b715, 0x3feef1a7373aa9cb,
    0x3feedea64c123422, 0x3feece086061892d, 0x3feebfdad5362a27, 0x3feeb42b569d4f82, 0x3feeab07dd485429,
    0x3feea47eb03a5585, 0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13,
    0x3feeace5422aa0db, 0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d, 0x3feee89f995ad3ad,
    0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069, 0x3fef5818dcfba487, 0x3fef7c97337b9b5f,
    0x3fefa4afa2a490da, 0x3fefd0765b6e4540};

BDPT_PF_INLINE double powf_log2(uint32_t ix) {
    const double A0 = 0x1.27616c9496e0bp-2, A1 = -0x1.71969a075c67ap-2, A2 = 0x1.ec70a6ca7baddp-2,
                 A3 = -0x1.7154748bef6c8p-1, A4 = 0x1.71547652ab82bp+0;
    uint32_t tmp = ix - 0x3f330000;
    int i = static_cast<int>((tmp >> 19) % 16);
    uint32_t top = tmp & 0xff800000;
    uint32_t iz = ix - top;
    int k = static_cast<int32_t>(top) >> 23;
    double z = static_cast<double>(pf_u2f(iz));
    double r = __builtin_fma(z, kPowfLog2Tab[i][0], -1.0);
    double y0 = kPowfLog2Tab[i][1] + static_cast<double>(k);
    double r2 = r * r;
    double y = __builtin_fma(A0, r, A1);
    double p = __builtin_fma(A2, r, A3);
    double r4 = r2 * r2;
    double q = __builtin_fma(A4, r, y0);
    q = __builtin_fma(p, r2, q);
    return __builtin_fma(y, r4, q);
}

BDPT_PF_INLINE float powf_exp2(double xd, uint32_t sign_bias) {
    // !TOINT_INTRINSICS path of glibc exp2_inline.
    const double shift = 0x1.8p+47;
    double kd = xd + shift;
    uint64_t ki = u_from_d(kd);
    kd -= shift;
    double r = xd - kd;
    uint64_t t = kExp2fTab[ki % 32];
    t += (ki + sign_bias) << 47;
    double s = d_from_u(t);
    double z = __builtin_fma(0x1.c6af84b912394p-5, r, 0x1.ebfce50fac4f3p-3);
    double r2 = r * r;
    double y = __builtin_fma(0x1.62e42ff0c52d6p-1, r, 1.0);
    y = __builtin_fma(z, r2, y);
    return static_cast<float>(y * s);
}

BDPT_PF_INLINE int powf_checkint(uint32_t iy) {
    int e = iy >> 23 & 0xff;
    if (e < 0x7f) return 0;
    if (e > 0x7f + 23) return 2;
    if (iy & ((1u << (0x7f + 23 - e)) - 1)) return 0;
    if (iy & (1u << (0x7f + 23 - e))) return 1;
    return 2;
}
BDPT_PF_INLINE bool powf_zeroinfnan(uint32_t i) { return 2 * i - 1 >= 2u * 0x7f800000 - 1; }
BDPT_PF_INLINE float powf_xflow(uint32_t sign, float y) { return (sign ? -y : y) * y; }

BDPT_PF_NOINLINE float powf_special(float x, float y, uint32_t ix, uint32_t iy, bool* done, uint32_t* ix_out,
                                    uint32_t* sign_bias) {
    *done = true;
    if (powf_zeroinfnan(iy)) {
        if (2 * iy == 0) return 1.0f;  // (signalling-NaN x is not produced by the BDPT path)
        if (ix == 0x3f800000) return 1.0f;
        if (2 * ix > 2u * 0x7f800000 || 2 * iy > 2u * 0x7f800000) return x + y;
        if (2 * ix == 2 * 0x3f800000) return 1.0f;
        if ((2 * ix < 2 * 0x3f800000) == !(iy & 0x80000000)) return 0.0f;
        return y * y;
    }
    if (powf_zeroinfnan(ix)) {
        float x2 = x * x;
        uint32_t sb = 0;
        if ((ix & 0x80000000) && powf_checkint(iy) == 1) {
            x2 = -x2;
            sb = 1;
        }
        if (2 * ix == 0 && (iy & 0x80000000)) return powf_xflow(sb, 1.0f) / 0.0f;
        return (iy & 0x80000000) ? 1 / x2 : x2;
    }
    *done = false;
    if (ix & 0x80000000) {
        int yint = powf_checkint(iy);
        if (yint == 0) {
            *done = true;
            return (x - x) / (x - x);
        }
        if (yint == 1) *sign_bias = 1u << 16;
        ix &= 0x7fffffff;
    }
    if (ix < 0x00800000) {
        ix = f2u(x * 0x1p23f);
        ix &= 0x7fffffff;
        ix -= 23 << 23;
    }
    *ix_out = ix;
    return 0.f;
}

BDPT_PF_ENTRY float glibc_powf(float x, float y) {
    uint32_t sign_bias = 0;
    uint32_t ix = f2u(x), iy = f2u(y);
    if (ix - 0x00800000 >= 0x7f800000 - 0x00800000 || powf_zeroinfnan(iy)) {
        bool done;
        float r = powf_special(x, y, ix, iy, &done, &ix, &sign_bias);
        if (done) return r;
    }
    double ylogx = static_cast<double>(y) * powf_log2(ix);
    if (((u_from_d(ylogx) >> 47) & 0xffff) >= (u_from_d(126.0) >> 47)) {
        if (ylogx > 0x1.fffffffd1d571p+6) return powf_xflow(sign_bias, 0x1p97f);
        if (ylogx <= -150.0) return powf_xflow(sign_bias, 0x1p-95f);
        if (ylogx < -149.0) return powf_xflow(sign_bias, 0x1.4p-75f);
    }
    return powf_exp2(ylogx, sign_bias);
}

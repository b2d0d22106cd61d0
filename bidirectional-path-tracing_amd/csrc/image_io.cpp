// 8-bit image files of bdpt_display's bytes (bdpt_amd.h): PNG and binary PPM, host only and without a
// dependency. Not in the reference, whose only output is the EXR.
//
// PNG (ISO/IEC 15948): the signature, IHDR (bit depth 8, colour type 2 for RGB or 6 for RGBA, no
// interlace), one IDAT and IEND. Every scanline is a filter-type byte 0 and the row's bytes. The IDAT
// data is a zlib stream (RFC 1950: header 0x78 0x01, Adler-32 of the raw data at the end) of deflate
// STORED blocks (RFC 1951 3.2.4: a header byte, LEN, ~LEN, LEN raw bytes; LEN at most 65535), so
// nothing is compressed and a decoder's inflate only copies. Chunk CRC-32 is the reflected 0xEDB88320
// polynomial over type and data.
//
// PPM: "P6\n<width> <height>\n255\n" and the RGB bytes, top row first: the header form the texture
// reader accepts (scene.cpp load_ppm_texture: "%*s %d %d %d%*c", no comments).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bdpt_amd.h"
#include "scene.hpp"

namespace bdpt {
namespace {

uint32_t crc32_of(const unsigned char* p, size_t n, uint32_t crc = 0) {
    static uint32_t table[256];
    static bool made = false;
    if (!made) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        made = true;
    }
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

void put_be32(std::vector<unsigned char>& b, uint32_t v) {
    for (int i = 3; i >= 0; i--) b.push_back(static_cast<unsigned char>(v >> (8 * i)));
}

// length, type, data, CRC of type + data; the data is what was appended to b after begin_chunk
size_t begin_chunk(std::vector<unsigned char>& b, const char type[4]) {
    const size_t at = b.size();
    put_be32(b, 0);
    b.insert(b.end(), type, type + 4);
    return at;
}
void end_chunk(std::vector<unsigned char>& b, size_t at) {
    const uint32_t len = static_cast<uint32_t>(b.size() - at - 8);
    for (int i = 0; i < 4; i++) b[at + i] = static_cast<unsigned char>(len >> (8 * (3 - i)));
    put_be32(b, crc32_of(b.data() + at + 4, len + 4));
}

bool check_image(const char* entry, const unsigned char* px, int W, int H, int channels, bool rgba_ok, std::string& err) {
    if (!px) err = std::string(entry) + ": pixels is NULL";
    else if (W < 1 || H < 1) err = std::string(entry) + ": width/height must be > 0";
    else if (channels != 3 && !(rgba_ok && channels == 4)) err = std::string(entry) + (rgba_ok ? ": channels must be 3 or 4" : ": channels must be 3");
    // (one IDAT chunk: its length is a 32-bit field)
    else if ((static_cast<uint64_t>(W) * channels + 1) * static_cast<uint64_t>(H) >= (1ull << 31)) err = std::string(entry) + ": the image is too large for one IDAT chunk";
    return err.empty();
}

bool encode_png(const unsigned char* px, int W, int H, int channels, std::vector<unsigned char>& out, std::string& err) {
    if (!check_image("bdpt_encode_png", px, W, H, channels, true, err)) return false;
    const size_t row = static_cast<size_t>(W) * channels, raw = (row + 1) * static_cast<size_t>(H);
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    out.assign(sig, sig + 8);
    out.reserve(8 + 25 + 12 + raw + 5 * (raw / 65535 + 1) + 6 + 12);
    size_t at = begin_chunk(out, "IHDR");
    put_be32(out, static_cast<uint32_t>(W));
    put_be32(out, static_cast<uint32_t>(H));
    const unsigned char tail[5] = {8, static_cast<unsigned char>(channels == 4 ? 6 : 2), 0, 0, 0};
    out.insert(out.end(), tail, tail + 5);
    end_chunk(out, at);

    at = begin_chunk(out, "IDAT");
    out.push_back(0x78), out.push_back(0x01);  // (deflate, 32 KiB window; a multiple of 31)
    // the raw stream, scanline by scanline, cut into stored blocks as it goes; Adler-32 alongside
    uint32_t a = 1, b = 0;
    size_t left = raw, in_block = 0;
    auto put = [&](const unsigned char* p, size_t n) {
        while (n) {
            if (in_block == 0) {
                const size_t len = left < 65535 ? left : 65535;
                out.push_back(left <= 65535 ? 1 : 0);  // BFINAL on the last block, BTYPE 00
                out.push_back(static_cast<unsigned char>(len & 0xff)), out.push_back(static_cast<unsigned char>(len >> 8));
                out.push_back(static_cast<unsigned char>(~len & 0xff)), out.push_back(static_cast<unsigned char>((~len >> 8) & 0xff));
                in_block = len;
            }
            const size_t take = n < in_block ? n : in_block;
            out.insert(out.end(), p, p + take);
            for (size_t i = 0; i < take; i++) {
                a += p[i];
                if (a >= 65521u) a -= 65521u;
                b += a;
                if (b >= 65521u) b -= 65521u;
            }
            p += take, n -= take, in_block -= take, left -= take;
        }
    };
    const unsigned char filter_none = 0;
    for (int y = 0; y < H; y++) {
        put(&filter_none, 1);
        put(px + row * static_cast<size_t>(y), row);
    }
    put_be32(out, (b << 16) | a);
    end_chunk(out, at);

    at = begin_chunk(out, "IEND");
    end_chunk(out, at);
    return true;
}

int write_file(const char* path, const unsigned char* head, size_t nhead, const unsigned char* body, size_t nbody) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return set_error(BDPT_ERR_IO, std::string("cannot open ") + path + " for writing");
    const size_t n = (nhead ? std::fwrite(head, 1, nhead, f) : 0) + (nbody ? std::fwrite(body, 1, nbody, f) : 0);
    const bool closed = std::fclose(f) == 0;
    if (n != nhead + nbody || !closed) return set_error(BDPT_ERR_IO, std::string("write failed: ") + path);
    return BDPT_OK;
}

}  // namespace
}  // namespace bdpt

extern "C" {

int bdpt_encode_png(const unsigned char* pixels, int32_t width, int32_t height, int32_t channels, unsigned char* out,
                    int64_t capacity, int64_t* size) {
    std::vector<unsigned char> buf;
    std::string err;
    if (!size) return bdpt::set_error(BDPT_ERR_INVALID, "bdpt_encode_png: size is NULL");
    if (!bdpt::encode_png(pixels, width, height, channels, buf, err)) return bdpt::set_error(BDPT_ERR_INVALID, err);
    *size = static_cast<int64_t>(buf.size());
    if (out) {
        if (capacity < static_cast<int64_t>(buf.size()))
            return bdpt::set_error(BDPT_ERR_INVALID, "bdpt_encode_png: output buffer too small");
        std::memcpy(out, buf.data(), buf.size());
    }
    return BDPT_OK;
}

int bdpt_save_png(const unsigned char* pixels, int32_t width, int32_t height, int32_t channels, const char* path) {
    std::vector<unsigned char> buf;
    std::string err;
    if (!path) return bdpt::set_error(BDPT_ERR_INVALID, "bdpt_save_png: path is NULL");
    if (!bdpt::encode_png(pixels, width, height, channels, buf, err)) return bdpt::set_error(BDPT_ERR_INVALID, err);
    return bdpt::write_file(path, buf.data(), buf.size(), nullptr, 0);
}

int bdpt_save_ppm(const unsigned char* rgb, int32_t width, int32_t height, const char* path) {
    std::string err;
    if (!path) return bdpt::set_error(BDPT_ERR_INVALID, "bdpt_save_ppm: path is NULL");
    if (!bdpt::check_image("bdpt_save_ppm", rgb, width, height, 3, false, err)) return bdpt::set_error(BDPT_ERR_INVALID, err);
    char head[64];
    const int n = std::snprintf(head, sizeof head, "P6\n%d %d\n255\n", width, height);
    return bdpt::write_file(path, reinterpret_cast<const unsigned char*>(head), static_cast<size_t>(n), rgb,
                            static_cast<size_t>(width) * height * 3);
}

}  // extern "C"

// C-ABI implementation (include/bdpt_amd.h): scene ingest, device context,
// frame and single-sample renders. Host code only; kernels live in
// bdpt_kernels.hip (the BDPT megakernel), sample_state.hip (single-sample
// kernels), pt_kernels.hip (path / direct) and kat_kernels.hip (per-function). No CPU fallback exists: every render runs the HIP kernels.
#include "../../include/bdpt_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "bdpt_device.hpp"
#include "scene.hpp"

namespace bdpt {
// The builds of the BDPT frame kernel (bdpt_kernels_<x>.hip; FrameBuild: bdpt_device.hpp)
extern FrameBuild frame_build, frame_build_tex, frame_build_rr, frame_build_rrc, frame_build_deep,
    frame_build_hbm, frame_build_split, frame_build_ng, frame_build_layers, frame_build_groups, frame_build_strat, frame_build_strat_unweighted,
    frame_build_groups_layers, frame_build_groups_strat, frame_build_groups_strat_unweighted, frame_build_pixels;
// sample_state.hip: the single-sample kernels (the caller's std::mt19937 state at sc.mt_ring)
hipError_t launch_sample(const dev::DevScene& sc, const dev::DevFrame& fr, float* splats, float* lvbuf, uint2* gstack,
                         const dev::Ray& ray, float* out, hipStream_t stream);
hipError_t launch_pt_sample(const dev::DevScene& sc, const dev::DevFrame& fr, const int32_t settings[8],
                            float4* levels, uint32_t* ring, uint2* gstack, const dev::Ray& ray, float* out,
                            unsigned long long* counters, hipStream_t stream, void* dparams);
// kat_kernels.hip: per-function entry points; the BSDF kernel also as the fast-weight frame
// kernels compile its functions (kat_kernels_fw.hip) and as the build without glossy lobes
// does (kat_kernels_ng.hip)
hipError_t launch_bsdf_kat(const dev::DevScene& sc, int mode, int64_t n, const int32_t* mat, const float* wo,
                           const float* x, float* out, hipStream_t st);
hipError_t launch_bsdf_kat_fw(const dev::DevScene& sc, int mode, int64_t n, const int32_t* mat, const float* wo,
                              const float* x, float* out, hipStream_t st);
hipError_t launch_bsdf_kat_ng(const dev::DevScene& sc, int mode, int64_t n, const int32_t* mat, const float* wo,
                              const float* x, float* out, hipStream_t st);
hipError_t launch_fresnel_kat(int64_t n, const float* in, float* out, hipStream_t st);
hipError_t launch_triangle_kat(int64_t n, const float* rays, const float* verts, float* out, hipStream_t st);
hipError_t launch_intersect_kat(const dev::DevScene& sc, int64_t n, int occlusion, const float* rays, const float* nrm,
                                const int32_t* otri, uint2* gstack, uint32_t nslots, float* out, hipStream_t st);
hipError_t launch_splat_kat(const dev::DevFrame& fr, int64_t n, const float* p, int32_t* xy, hipStream_t st);
// kat_leaf_defer.hip: the closest hit with the reference-leaf check deferred to the walk's winner
hipError_t launch_intersect_defer(const dev::DevScene& sc, int64_t n, int by_id, int force, const float* rays,
                                  const float* nrm, const int32_t* otri, uint2* gstack, uint32_t nslots, float* out,
                                  int32_t* rewalked, hipStream_t st);
// kat_sampling.hip: the sampling side per function, and with the fast weights (kat_sampling_fw.hip)
hipError_t launch_sampling_kat(const dev::DevScene& sc, const dev::DevFrame& fr, int fn, int nin, int nout, int64_t n,
                               const uint32_t* in, uint32_t* out, hipStream_t st);
hipError_t launch_sampling_kat_fw(const dev::DevScene& sc, const dev::DevFrame& fr, int fn, int nin, int nout,
                                  int64_t n, const uint32_t* in, uint32_t* out, hipStream_t st);
// sample_state_tex.hip: the single-sample kernel for scenes with bitmap textures
hipError_t launch_sample_tex(const dev::DevScene& sc, const dev::DevFrame& fr, float* splats, float* lvbuf,
                             uint2* gstack, const dev::Ray& ray, float* out, hipStream_t stream);
size_t pt_params_bytes();
int pt_blocks_per_cu(size_t dyn_lds);
hipError_t launch_pt(const dev::DevScene& sc, const dev::DevFrame& fr, const int32_t settings[8], float* fb,
                     float4* levels, uint32_t* ring, uint2* gstack, uint32_t nslots, unsigned long long* work,
                     unsigned long long* counters, int grid, hipStream_t stream, void* dparams);
hipError_t launch_math_check(int32_t fn, const float* x, const float* y, float* out, int64_t n, hipStream_t st);
// math_check_fw.hip: the same with BDPT_FAST_WEIGHTS 1 (the weight operations' hardware forms)
hipError_t launch_math_check_fw(int32_t fn, const float* x, const float* y, float* out, int64_t n, hipStream_t st);
// aov_kernels.hip: first-hit feature buffers and the a-trous filter
hipError_t launch_aov(const dev::DevScene& sc, const dev::DevFrame& fr, const void* mats, float* aov, uint2* gstack,
                      uint32_t nslots, hipStream_t st);
hipError_t launch_denoise_prepare(int W, int H, const float* color, const float* aov, float norm, int demodulate,
                                  void* guide, void* img, hipStream_t st);
hipError_t launch_denoise_scale(size_t n, const float* color, float norm, float* out, hipStream_t st);
hipError_t launch_denoise_iter(int W, int H, int step, float inv_c, float inv_n, float sigma_z, int demodulate,
                               const void* guide, const void* src, void* dst, float* out, bool last, hipStream_t st);
// aov_kernels.hip: the filter for many planes, denoise_planes_chunk() planes per launch
int denoise_planes_chunk();
hipError_t launch_planes_sum(const float* planes, size_t n, int n_planes, float scale, float* out, hipStream_t st);
hipError_t launch_denoise_planes_prepare(int W, int H, const float* planes, int cnt, float norm, int demodulate,
                                         const void* guide, void* img, hipStream_t st);
hipError_t launch_denoise_planes_iter(int W, int H, int step, float inv_c, float inv_n, float sigma_z, int demodulate,
                                      int cnt, const void* guide, const void* b, const void* src, void* dst, float* out,
                                      bool last, hipStream_t st);
// aov_kernels.hip: per-pixel sum and variance across K batch planes of n floats (c = K / (K - 1); sum may be null)
hipError_t launch_batch_moments(const float* planes, size_t n, int K, float c, float* sum, float* var, hipStream_t st);
// aov_kernels.hip: the a-trous filter with a variance-normalised colour weight (the variance rides in the images' .w)
// adaptive_kernels.hip: adaptive sampling's state (bdpt_adaptive_resolve, bdpt_adaptive_select)
hipError_t launch_adaptive_resolve(const float* planes, const int32_t* m, size_t n, int K, int spp, float t, float c,
                                   float* sum, float* var, hipStream_t st);
size_t adaptive_select_scratch_bytes(size_t pixels);
hipError_t launch_adaptive_select(const float* S, const float* var, int W, int H, float thr, float eps, int step, int m_max,
                                  int dilate, int32_t* m, int32_t* list, int32_t* count, void* scratch, hipStream_t st);
hipError_t launch_adaptive_start(size_t pixels, int step, int32_t* m, int32_t* list, hipStream_t st);
hipError_t launch_adaptive_samples(size_t pixels, int K, const int32_t* m, int32_t* samples, hipStream_t st);
// temporal_kernels.hip: temporal accumulation (bdpt_reproject)
hipError_t launch_reproject(const dev::DevFrame& fr, const CameraConstants& prev, float norm, float n_c, float max_history,
                            float sigma_normal, float sigma_depth, float min_weight, float clamp_sigma, int demodulate,
                            const float* color, const float* aov, const float* hist_in, float* out, float* hist_out,
                            hipStream_t st);
hipError_t launch_denoise_var_prepare(int W, int H, const float* color, const float* var, const float* aov, float norm,
                                      int demodulate, void* guide, void* img, hipStream_t st);
hipError_t launch_denoise_var_blur(int W, int H, const void* src, void* dst, float* out_var, hipStream_t st);
hipError_t launch_denoise_var_iter(int W, int H, int step, float sc2, float inv_n, float sigma_z, int demodulate,
                                   const void* guide, const void* src, void* dst, float* out, float* out_var, bool last,
                                   hipStream_t st);
// display_kernels.hip: display output (bdpt_meter, bdpt_display)
hipError_t launch_display(const float* color, const float* thresholds, const uint32_t* meter, float norm, float exposure,
                          float white, int tone, int channels, size_t N, unsigned char* out, hipStream_t st);
hipError_t launch_meter(const float* color, const float* aov, const uint32_t* prev, float norm, float key, int key_permille,
                        int white_permille, float rate, float fallback_exposure, float fallback_white, size_t N,
                        uint32_t* hist, uint32_t* out, hipStream_t st);
// aov_kernels.hip: a masked sum of path-length layers (planes of n floats)
hipError_t launch_layers_compose(const float* layers, size_t n, uint64_t mask, float* out, hipStream_t st);
// aov_kernels.hip: light-group planes (n floats each) recombined with per-group RGB gains (host, n_groups x 3)
hipError_t launch_relight(const float* planes, size_t n, int n_groups, const float* gains, float* out, hipStream_t st);
// aov_kernels.hip: n_groups * n_inner crossed planes (n floats each) recombined with per-group RGB gains (host,
// n_groups x 3) and per-inner-plane weights (a device table of n_inner floats)
hipError_t launch_group_planes_combine(const float* planes, size_t n, int n_groups, int n_inner, const float* gains,
                                       const float* weights, float* out, hipStream_t st);
// aov_kernels.hip: the contact sheet of n_s x n_t strategy planes (gains: a device table of n_s * n_t x 3 floats, or null)
hipError_t launch_strategies_sheet(const float* planes, int n_s, int n_t, int W, int H, const float* gains, float* out,
                                   hipStream_t st);
}  // namespace bdpt

using namespace bdpt;

namespace {
thread_local std::string g_error;

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

// Debugging knobs that change what a render computes (BDPT_SAMPLE_RANGE: a part
// of the frame; BDPT_GRAZE_CODES=0: the plain near-cull rule, not exact on smooth
// meshes) are read only when BDPT_DEBUG_KNOBS=1 is set too (tools/rr_find.py, A/B
// sweeps); set without it they are ignored with one warning on stderr.
const char* debug_knob(const char* name) {
    const char* v = std::getenv(name);
    if (!v) return nullptr;
    const char* on = std::getenv("BDPT_DEBUG_KNOBS");
    if (on && *on == '1') return v;
    static bool warned = false;
    if (!warned) {
        warned = true;
        std::fprintf(stderr, "bdpt_amd: %s is a debugging knob, ignored without BDPT_DEBUG_KNOBS=1\n", name);
    }
    return nullptr;
}

static bool leaf_recheck_knob() {
    const char* e = debug_knob("BDPT_LEAF_RECHECK");
    return e && *e == '1';
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail(BDPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The owner of one device allocation; every device pointer of this file lives in one.
// reserve() only grows and keeps no contents. Before it frees a live allocation it waits for
// the device: work in flight on any stream may still read the old memory. That wait is the
// one growth policy here; growth happens on a first call or a larger frame, never per frame
// in steady state. A reserve that fails leaves the buffer empty.
template <class T>
class DevBuf {
   public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = p_ ? hipDeviceSynchronize() : hipSuccess;
        release();
        if (e == hipSuccess) e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else bytes_ = bytes;
        return e;
    }
    T* get() const { return static_cast<T*>(p_); }
    operator T*() const { return get(); }

   private:
    void release() {
        if (p_) (void)hipFree(p_);  // (teardown is best effort: nobody can act on an error here)
        p_ = nullptr, bytes_ = 0;
    }
    void* p_ = nullptr;
    size_t bytes_ = 0;  // capacity
};

constexpr int kCounterWords = BDPT_NUM_COUNTERS + 3 + 4;  // sums, the counting pass's 3 maxima (Counts::m), the task histogram (Counts::q)
constexpr uint32_t kTaskCap = 256;  // shadow-ray tasks per wave ring (a power of two; DevFrame::tasks)
constexpr int kLazyRrDepth = 28;  // lazy MT19937 covers 10 + 8 * 27 = 226 < 227 draws
// Short subpaths run the BDPT_SPLIT_CONTINUE build (bdpt_kernels_split.hip): the
// ST_DEFER step it removes is one loop slot of the ~(rrDepth + 1)^2 / 2 a sample
// takes, while its separate light / eye continuation bodies cost every shading
// step (measured, DESIGN.md §5: Caustic rrDepth 2 / 3 / 4 / 8: +11.4 / +1.1 / -1.5 / -3.7 %,
// HardLight rrDepth 2 / 3 / 4 / 5: +12.5 / +4.4 / +1.2 / -0.2 %).
// BDPT_SPLIT_MAX_RR overrides the threshold (0: never).
constexpr int kSplitMaxRrDepth = 3;
constexpr int64_t kDeepSceneTris = 262144;  // scenes from this many triangles shade at 36 ready lanes (their walks are longer)
static bool use_split_build(int rr_depth) {
    const char* e = std::getenv("BDPT_SPLIT_MAX_RR");  // read per render (tests force either build)
    return rr_depth <= (e ? std::atoi(e) : kSplitMaxRrDepth);
}
// Russian-roulette continuation pass (bdpt_kernels.hip, park_lane), opt-in: a
// light or eye walk deeper than BDPT_PARK_DEPTH bounces (default 0: off) leaves
// the megakernel for the chain kernel (one wave per sample), which walks its
// delta chain with the whole wave; BDPT_PARK_ROUNDS (default 4) chain + resume
// rounds follow the frame (the last resume keeps every walk in the megakernel).
// Measured slower than walking a lone trapped lane with its own wave inside the
// megakernel (BDPT_COOP_ALONE, the default): Caustic 512^2 x 256 68.6 s vs 45.3 s —
// each round waits for its longest chain, so two long chains of different
// samples that park in different rounds run one after the other.
static int park_depth_setting() {
    const char* e = std::getenv("BDPT_PARK_DEPTH");
    return e ? std::atoi(e) : 0;
}
static int park_rounds_setting() {
    const char* e = std::getenv("BDPT_PARK_ROUNDS");
    return e ? std::max(1, std::atoi(e)) : 4;
}
// One wave per parked walk (grid-stride beyond): a frame parks ~2 400 walks of
// ~180 k bounces on average (Caustic 512^2 x 256), which run side by side.
constexpr int kChainGrid = 8192;
constexpr int kMaxRrDepth = 1024;  // beyond 28 the megakernel continues MT19937 from an HBM ring
// Russian roulette (NO_RR = 0): subpaths are unbounded in the reference (a light
// subpath trapped by total internal reflection in the Caustic sphere was measured
// at 67 714 bounces). Here the light-vertex store of a lane slot holds
// max(kRrLightVerts, rrDepth - 1) vertices (64 B each; the shipped scenes store at
// most 36), and a walk past kRrDepthGuard bounces is a hang guard; a sample that
// meets either is counted (bdpt_stats.capped_samples) and the host render fails
// rather than return a different image.
constexpr int kRrLightVerts = 255;
// A Caustic light subpath trapped in the glass sphere by total internal reflection
// runs for millions of bounces (the oracle over a 512^2 x 256 frame: 2.7 M light /
// 2.1 M eye bounces in one sample); the guard sits an order of magnitude above.
constexpr int kRrDepthGuard = 1 << 25;
// A frame kept as several planes (path-length layers, light groups, strategy images): the most
// planes of each kind, and the limit they share. The messages take their figures from here.
constexpr int kMaxLayers = 64;  // a layer mask is one 64-bit word (bdpt_layers_compose)
constexpr int kMaxGroups = 64;  // the relight kernel's gains are a kernel argument (bdpt_light_groups_relight)
constexpr int kMaxStratS = kLazyRrDepth + 1, kMaxStratT = kLazyRrDepth;  // every strategy of rr_depth 28
// a contribution's plane and pixel travel as one index in the task record's 30-bit pixel field
constexpr int kPlanePixelBits = 30;
constexpr int64_t kMaxPlanePixels = int64_t{1} << kPlanePixelBits;
const std::string kBelowPlanePixels = "below 2^" + std::to_string(kPlanePixelBits);
std::string in_range(int max) { return " must be in [1, " + std::to_string(max) + "]"; }
}  // namespace

// Error reporting shared with the other C-ABI translation units (exr_io.cpp, toml_config.cpp).
int bdpt::set_error(int code, const std::string& msg) { return fail(code, msg); }

// The state of std::mt19937(seed) after `draws` outputs, as libstdc++'s
// operator<< writes it: _M_x[0..623], then _M_p.
static void mt19937_state(uint32_t seed, int64_t draws, uint32_t st[BDPT_MT19937_WORDS]) {
    std::mt19937 g(seed);
    g.discard(static_cast<unsigned long long>(draws));
    std::ostringstream os;
    os << g;
    std::istringstream is(os.str());
    for (int i = 0; i < BDPT_MT19937_WORDS; i++) {
        unsigned long long v = 0;
        is >> v;
        st[i] = static_cast<uint32_t>(v);
    }
}

struct bdpt_scene {
    HostScene host;
    DeviceLayout layout;
};

// The context's stream and events. A base of bdpt_ctx, so that they are destroyed after its
// members: the buffers are freed first.
struct CtxStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // cross-stream ordering of the context's buffers: the last call's stream and
    // an event recorded on it after that call's work
    hipEvent_t last_use = nullptr;
    hipStream_t last_stream = nullptr;
    bool used = false;
    CtxStream() = default;
    CtxStream(const CtxStream&) = delete;
    CtxStream& operator=(const CtxStream&) = delete;
    ~CtxStream() {  // best effort, as every teardown
        for (hipEvent_t e : {last_use, ev0, ev1})
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct bdpt_ctx : CtxStream {
    const char* last_kernel = "";  // the frame kernel build the last render launched (bdpt_last_kernel)
    int last_kernel_glossy = 1;    // 0: that build has no Mixture / Phong lobes (bdpt_last_kernel_glossy)
    int device = 0;
    int cus = 0;
    int grid = 0;
    // scene arrays
    std::vector<DevBuf<void>> allocs;
    dev::DevScene sc{};
    int max_depth = 0;
    bool tri_tree = false;              // traversal boxes padded (wide_bvh.hpp kTriBoxPad)
    int64_t wnode_bytes = 0;            // the 4-wide node array (load_wnode_nf: 32-bit offsets into it)
    double box_lo[3] = {}, box_hi[3] = {};  // scene bounds (the reference BVH's root box)
    int64_t scene_bytes = 0;
    int64_t ntri = 0;  // triangles (shade records)
    uint32_t lds_words_base = 0;  // dynamic LDS words without the emitter faces / CDFs
    // work buffers
    DevBuf<unsigned long long> work;      // work counter
    DevBuf<unsigned long long> counters;  // kCounters
    DevBuf<float> lv;
    DevBuf<uint2> gstack;  // traversal-stack overflow beyond the LDS part
    uint32_t nslots = 0;
    DevBuf<float> tmp_fb;  // the host entries' staging buffer (stage_host)
    DevBuf<float> sample_out;
    DevBuf<void> dparams;  // kernel parameter block (filled in stream order per launch)
    // path tracer (pt_kernels.hip): level stacks, generator rings, parameter block
    int pt_grid = 0;
    uint32_t pt_nslots = 0;
    DevBuf<float4> pt_levels;
    DevBuf<uint32_t> pt_ring;
    DevBuf<uint32_t> mt_ring;  // BDPT megakernel: MT19937 continuation past 227 draws (rrDepth > 28, RR)
    DevBuf<uint32_t> park;     // Russian roulette: continuation records + parked-slot list (DevFrame::park)
    DevBuf<float4> tasks;      // per-wave shadow-ray task rings (DevFrame::tasks; read by BDPT_HELP builds)
    uint32_t task_cap = 0;        // their capacity (tasks per wave, a power of two)
    bool textured = false;        // the scene has bitmap textures: bdpt_render runs bdpt_kernels_tex.hip
    std::vector<uint8_t> mat_textured;  // per material: it reads a map (bdpt_bsdf_* carry no hit to look one up)
    bool has_glass = false;       // a GlassBSDF material: Russian-roulette renders run bdpt_kernels_rrc.hip
    bool has_glossy = false;      // a Mixture / Phong record in the device table (after device_bsdfs)
    bool has_null = false;        // a null BSDF (illum 5): not delta, not diffuse
    // bdpt_render_light_groups: the call's emitter -> group table (DevFrame::emitter_group) and the
    // host copy it is uploaded from (the caller's array is not read after the call returns)
    DevBuf<int32_t> emitter_group;
    std::vector<int32_t> emitter_group_host;
    // bdpt_strategies_sheet: the call's per-plane RGB gains, likewise
    DevBuf<float> sheet_gains;
    std::vector<float> sheet_gains_host;
    DevBuf<int32_t> row_order;  // bdpt_set_row_order (device copy; DevFrame::row_order)
    int32_t row_order_n = 0;    // its row count (0: top to bottom)
    DevBuf<int32_t> pixel_list;  // bdpt_render_pixels_host: the device copy of the caller's list (DevFrame::pixel_list)
    // adaptive sampling (bdpt_render_adaptive): the K plane pairs, samples per batch and pixel, the pass's
    // list, its count, the select kernels' scratch; the host forms' staging; the recorded lists
    DevBuf<float> ad_planes;
    DevBuf<int32_t> ad_m, ad_list, ad_count;
    DevBuf<void> ad_scratch, ad_stage;
    std::vector<int32_t> ad_pass_lists;
    DevBuf<unsigned long long> row_cost;  // counting renders: queries per local row (DevFrame::row_cost)
    int32_t row_cost_n = 0;               // the rows of the last counting render
    unsigned long long work_init = 0;  // BDPT_SAMPLE_RANGE's first sample (host copy for the async upload)
    DevBuf<uint32_t> capped;            // samples that met the Russian-roulette bounds, per call
    DevBuf<unsigned long long> diag;    // the BDPT frame kernel's timeline (dev::kDiag*)
    bool diag_pending = false;    // the last call was a BDPT frame render (diag is its)
    int wall_khz = 100000;        // s_memrealtime rate
    DevBuf<void> pt_dparams;
    // single-sample calls: the caller's std::mt19937 state and the splat list
    DevBuf<uint32_t> mt_state;  // BDPT_MT19937_WORDS
    DevBuf<float> splat_list;   // header (count, capacity) + capacity (pixel, r, g, b) records
    int32_t splat_cap = 0;
    // feature buffers (bdpt_render_aov): per material (Kd, albedo mode) (Ks, 0) of the records as
    // ingested, and for a scene without maps a table of "no map" records for shade_hit's lookup
    DevBuf<void> aov_mats;
    DevBuf<float4> aov_no_tex;
    // filter (bdpt_denoise): packed guides (2 float4 per pixel) and the ping-pong images (float4
    // per pixel each), reserved together at first use and when a larger frame comes
    DevBuf<void> dn_guide, dn_img[2];
    size_t dn_pixels = 0;  // the frame all three hold (0 after a failed reserve)
    // filter for many planes (bdpt_denoise_planes): packed guides, the guide's images B_0 .. B_7
    // (SHARED mode) and the ping-pong pair of the planes in flight; each grows on its own
    DevBuf<void> dnp_guide, dnp_traj, dnp_img[2];
    // display output (bdpt_meter, bdpt_display): the meter's global histogram (zeroed per call), the three
    // encodes' threshold tables (256 floats each, uploaded at the first display call), the host forms' staging
    DevBuf<uint32_t> meter_hist;
    DevBuf<float> display_tables;
    bool display_tables_ready = false;
    DevBuf<void> display_stage;
    // stats of the last render
    bool pending_timing = false;
    bdpt_stats stats{};
};

// Calls on one context are ordered even when they use different streams: a
// call first makes its stream wait for the previous call's work (an event
// recorded at that call's end), since all calls share the context's buffers.
static int begin_use(bdpt_ctx* c, hipStream_t st) {
    if (c->used && c->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->last_use, 0));
    return BDPT_OK;
}
static int end_use(bdpt_ctx* c, hipStream_t st) {
    HIP_TRY(hipEventRecord(c->last_use, st));
    c->last_stream = st;
    c->used = true;
    return BDPT_OK;
}

// The timed part of a call (frame renders, feature buffers, the filter): its counters start at
// zero, ev0 / ev1 bracket its launches for kernel_ms, and its stats replace the last call's.
// diag_pending: the call was a BDPT frame render, the timeline in c->diag is its.
static int begin_timed(bdpt_ctx* c, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * kCounterWords, st));
    HIP_TRY(hipMemsetAsync(c->capped, 0, sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->ev0, st));
    return BDPT_OK;
}
static int end_timed(bdpt_ctx* c, hipStream_t st, int64_t samples, int64_t launches, bool diag_pending = false) {
    HIP_TRY(hipEventRecord(c->ev1, st));
    if (int rc = end_use(c, st)) return rc;
    c->pending_timing = true;
    c->diag_pending = diag_pending;
    c->stats = bdpt_stats{};
    c->stats.samples = samples;
    c->stats.launches = launches;
    return BDPT_OK;
}

// A scene array: the context owns it (allocs, counted in scene_bytes), dst is the pointer the kernels read.
template <class P>
static int upload(bdpt_ctx* c, const void* src, size_t bytes, P& dst) {
    if (bytes == 0) bytes = 16;
    DevBuf<void> b;
    HIP_TRY(b.reserve(bytes));
    if (src) HIP_TRY(hipMemcpy(b, src, bytes, hipMemcpyHostToDevice));
    dst = static_cast<P>(b.get());
    c->allocs.push_back(std::move(b));
    c->scene_bytes += static_cast<int64_t>(bytes);
    return BDPT_OK;
}

// The host form of a frame entry: the caller's n floats staged in tmp_fb, the device entry
// run on them on the context's stream (run(device pointer)), the result copied back and
// waited for. What an entry checks before and after stays with the entry.
template <class Run>
static int stage_host(bdpt_ctx* c, float* host, size_t n, Run run) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->tmp_fb.reserve(n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(c->tmp_fb, host, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = run(c->tmp_fb.get())) return rc;
    HIP_TRY(hipMemcpyAsync(host, c->tmp_fb, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// The device part of a combine entry (bdpt_layers_compose, bdpt_light_groups_relight,
// bdpt_strategies_sheet, bdpt_group_planes_combine) once its arguments are accepted: one launch on
// the call's stream, timed as a call of its own. table (null: none): the sheet's ntable gains or the
// crossed combine's ntable weights, which reach the device in stream order from the context's own
// host copy; launch(device table or null, stream).
template <class Launch>
static int combine_planes(bdpt_ctx* c, void* hip_stream, const float* table, size_t ntable, Launch launch) {
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = begin_use(c, st)) return rc;
    const float* dtable = nullptr;
    if (table) {
        c->sheet_gains_host.assign(table, table + ntable);
        HIP_TRY(c->sheet_gains.reserve(sizeof(float) * 3 * kMaxStratS * kMaxStratT));  // (the largest table, once)
        HIP_TRY(hipMemcpyAsync(c->sheet_gains, c->sheet_gains_host.data(), sizeof(float) * ntable, hipMemcpyHostToDevice, st));
        dtable = c->sheet_gains;
    }
    if (int rc = begin_timed(c, st)) return rc;
    HIP_TRY(launch(dtable, st));
    return end_timed(c, st, 0, 1);
}

// The LDS tables with the emitter faces (5 float4 each) and CDFs appended to `base` words:
// their word offsets, and the total (16-byte rounded parts; dev_scene.hpp scene_tables_to_lds).
constexpr uint32_t kLdsBudget = 24u * 1024u;  // bytes of dynamic LDS the scene tables may take
static uint32_t emitter_lds_layout(const dev::DevScene& sc, uint32_t base, uint32_t& etri, uint32_t& ecdf) {
    auto up4 = [](uint32_t w) { return (w + 3u) & ~3u; };
    etri = base;
    ecdf = up4(etri + 20u * static_cast<uint32_t>(sc.n_etri));
    return up4(ecdf + static_cast<uint32_t>(sc.n_ecdf));
}

// Host arrays in, device run, host arrays out (the per-function entry points): a device array
// of the call, filled from src on the context's stream (src null: an output, left as allocated).
template <class T>
static int kat_in(bdpt_ctx* c, DevBuf<T>& b, const T* src, size_t bytes) {
    HIP_TRY(b.reserve(std::max<size_t>(bytes, 16)));
    if (src && bytes) HIP_TRY(hipMemcpyAsync(b, src, bytes, hipMemcpyHostToDevice, c->stream));
    return BDPT_OK;
}

// The BSDF records as the kernels read them. A MixtureBSDF with Ks == 0, scale
// == 1 and a finite exponent >= 0 (so specw == 0) returns DiffuseBSDF's values
// bit for bit (mixture.h:59-151 against diffuse.h:35-61): eval adds
// (0 * (n + 2)) * INV_TWOPI * powf(c, n) = +0 (c in [0, 1], so powf is
// finite) to Kd * INV_PI and multiplies by 1; pdf is pdfPhong * 0 + pdfDiffuse
// * 1 with a finite pdfPhong; sample takes the diffuse branch (u.x < 0 never
// holds) with (u.x - 0) / (1 - 0) == u.x. The kernels run it as diffuse, so a
// wave whose lanes shade both kinds runs one branch instead of two.
// BDPT_KEEP_MIXTURE=1 keeps the record as loaded (the A/B of DESIGN.md).
// A material with a specular map keeps its kind: its Ks is the texel's, not the record's.
static std::vector<BsdfRecord> device_bsdfs(const std::vector<BsdfRecord>& in, const std::vector<int32_t>& mat_tex) {
    std::vector<BsdfRecord> out = in;
    const char* keep = std::getenv("BDPT_KEEP_MIXTURE");
    if (keep && *keep == '1') return out;
    for (size_t m = 0; m < out.size(); m++) {
        BsdfRecord& b = out[m];
        const bool ks_map = 2 * m + 1 < mat_tex.size() && mat_tex[2 * m + 1] >= 0;
        const bool ks0 = b.ks[0] == 0.f && b.ks[1] == 0.f && b.ks[2] == 0.f && !ks_map;
        if (b.kind == BSDF_MIXTURE && ks0 && b.scale == 1.f && b.specw == 0.f && std::isfinite(b.exponent) &&
            b.exponent >= 0.f)
            b.kind = BSDF_DIFFUSE;  // type keeps the reference's flags (only its delta bits are read)
    }
    return out;
}

// Near-cull exemption margin of a triangle (cull_near_for, bdpt_path.hpp; DESIGN.md
// §2 item 5). The frames exempt a query that leaves a surface at |cos| < kGrazeCos
// to the triangle's GEOMETRIC plane; at run time they only have the interpolated
// shading normal n_s. Every n_s of the triangle is a normalized positive
// combination of its corner normals, so it lies in their cone: if each corner
// normal is within angle th of sgn * n_g (one side of the plane), |n_s - sgn * n_g|
// <= 2 sin(th / 2) and |dot(d, n_g)| < kGrazeCos implies |dot(d, n_s)| < kGrazeCos +
// 2 sin(th / 2). The code is that margin in units of 1/64, rounded up (with 1e-5 for
// the float normalization of n_s); 0 for flat triangles (corner normals parallel to
// n_g: n_s is then n_g's own direction), 255 (always exempt) for corner normals on
// both sides of the plane, zero normals or degenerate triangles.
static uint32_t graze_code(const float* v0, const float* v1, const float* v2, const float* const n[3]) {
    double e1[3], e2[3];
    for (int a = 0; a < 3; a++) e1[a] = double(v1[a]) - v0[a], e2[a] = double(v2[a]) - v0[a];
    double g[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double gl = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    if (!(gl > 0.0) || !std::isfinite(gl)) return 255u;
    {  // A sliver: the near cull's argument (dev_traverse.hpp kGrazeCos) needs every corner above ~0.35
       // degrees; below it the triangle test's t on a coplanar origin is noise the reference may accept
       // at any |cos|, so queries leaving such a triangle always walk without the near cull.
        constexpr double kMinCornerSin = 6.2e-3;  // sin(0.355 degrees)
        double e3[3];
        for (int a = 0; a < 3; a++) e3[a] = double(v2[a]) - v1[a];
        const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
        const double l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        const double l3 = std::sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
        // sin of the corner between two sides = |cross| / (their lengths); |cross| is gl for every pair
        const double smallest = gl / std::max(l1 * l2, std::max(l1 * l3, l2 * l3));
        if (!(smallest >= kMinCornerSin)) return 255u;
    }
    double worst = 0.0;  // max over corners of 2 sin(th / 2) = |n_k - sgn n_g|
    int sgn = 0;
    for (int k = 0; k < 3; k++) {
        const double nl = std::sqrt(double(n[k][0]) * n[k][0] + double(n[k][1]) * n[k][1] + double(n[k][2]) * n[k][2]);
        if (!(nl > 0.0) || !std::isfinite(nl)) return 255u;
        const double c = (n[k][0] * g[0] + n[k][1] * g[1] + n[k][2] * g[2]) / (nl * gl);
        const int s = c > 0.0 ? 1 : c < 0.0 ? -1 : 0;
        if (s == 0 || (sgn != 0 && s != sgn)) return 255u;
        sgn = s;
        worst = std::max(worst, std::sqrt(std::max(0.0, 2.0 - 2.0 * std::fabs(c))));
    }
    if (worst < 1e-9) return 0u;
    const double code = std::ceil((worst + 1e-5) * 64.0);
    return code >= 255.0 ? 255u : static_cast<uint32_t>(code);
}

// The shading records as uploaded (bdpt_types.h kShadeStride): the host five
// (n0, mat) (n1, shape) (n2, prim) (v1) (v2), + (v0) in the wide layout, with the
// triangle's graze code in bits 24..31 of the shape word (shape ids < 2^24) and, with
// leaf_box, the triangle's reference leaf box or leaf id in the last two slots (below).
static std::vector<float4_t> device_shade(const DeviceLayout& L, bool leaf_box = true) {
    const char* gz = debug_knob("BDPT_GRAZE_CODES");  // "0": every code 0 (the plain |cos| < 0.02 test; A/B only)
    const bool codes = !(gz && *gz == '0');
    const size_t ntri = L.shade.size() / 5;
    std::vector<float4_t> out(kShadeStride * ntri, float4_t{0.f, 0.f, 0.f, 0.f});
    for (size_t i = 0; i < ntri; i++) {
        for (int q = 0; q < 5; q++) out[kShadeStride * i + q] = L.shade[5 * i + q];
        if (kShadeStride > kShadeV0) out[kShadeStride * i + kShadeV0] = L.tri[3 * i];
        if (L.textured() && kShadeStride >= kShadeSt + 2) {  // the corners' texture coordinates, in the same line
            const float* st = &L.tri_st[6 * i];
            out[kShadeStride * i + kShadeSt] = {st[0], st[1], st[2], st[3]};
            out[kShadeStride * i + kShadeSt + 1] = {st[4], st[5], 0.f, 0.f};
        }
        const float4_t* s = &L.shade[5 * i];
        const float v0[3] = {L.tri[3 * i].x, L.tri[3 * i].y, L.tri[3 * i].z};
        const float v1[3] = {s[3].x, s[3].y, s[3].z}, v2[3] = {s[4].x, s[4].y, s[4].z};
        const float n0[3] = {s[0].x, s[0].y, s[0].z}, n1[3] = {s[1].x, s[1].y, s[1].z}, n2[3] = {s[2].x, s[2].y, s[2].z};
        const float* const n[3] = {n0, n1, n2};
        uint32_t shape;
        std::memcpy(&shape, &s[1].w, 4);
        if (codes) shape |= graze_code(v0, v1, v2, n) << 24;
        std::memcpy(&out[kShadeStride * i + 1].w, &shape, 4);
    }
    // The triangle's reference leaf box (kShadeBox), for the deferred leaf check of a closest hit:
    // a traversal triangle names its shade record (v0's w) and its reference leaf (e1's w). The
    // box's two vectors go into the record's free slots; where the texture coordinates hold those,
    // the leaf id goes into their free last word and the kernel reads lbox.
    for (size_t k = 0; leaf_box && kShadeStride >= kShadeBox + 2 && 3 * k + 1 < L.wtri.size(); k++) {
        uint32_t i, leaf;
        std::memcpy(&i, &L.wtri[3 * k].w, 4);
        std::memcpy(&leaf, &L.wtri[3 * k + 1].w, 4);
        if (i >= ntri || 2 * static_cast<size_t>(leaf) + 1 >= L.lbox.size()) continue;
        if (L.textured()) {
            std::memcpy(&out[kShadeStride * i + kShadeBox + 1].w, &leaf, 4);
        } else {
            out[kShadeStride * i + kShadeBox] = L.lbox[2 * static_cast<size_t>(leaf)];
            out[kShadeStride * i + kShadeBox + 1] = L.lbox[2 * static_cast<size_t>(leaf) + 1];
        }
    }
    return out;
}

// The emitter faces as uploaded: 5 float4 per face (v0 v1 v2 n0 n1 n2, 18 floats)
// with the face's graze code in the first free word (the first light ray leaves it).
static std::vector<float4_t> device_emit_tri(const DeviceLayout& L) {
    std::vector<float4_t> out = L.emit_tri;
    for (size_t f = 0; f + 5 <= out.size(); f += 5) {
        float w[20];
        std::memcpy(w, &out[f], sizeof(w));
        const float* const n[3] = {w + 9, w + 12, w + 15};
        const uint32_t code = graze_code(w, w + 3, w + 6, n);
        std::memcpy(&out[f + 4].z, &code, 4);
    }
    return out;
}

extern "C" {

const char* bdpt_last_error(void) { return g_error.c_str(); }
const char* bdpt_version(void) { return "bdpt_amd 0.1 (gfx950 megakernel v0)"; }

int bdpt_scene_load_obj(const char* obj_path, bdpt_scene** out) {
    if (!obj_path || !out) return fail(BDPT_ERR_INVALID, "null argument");
    auto s = std::make_unique<bdpt_scene>();
    std::string err;
    int code = BDPT_ERR_IO;
    if (!load_obj_scene(obj_path, s->host, err, &code)) return fail(code, err);
    if (!build_device_layout(s->host, s->layout, err)) return fail(BDPT_ERR_INVALID, err);
    *out = s.release();
    return BDPT_OK;
}

int bdpt_scene_create_textured(const bdpt_scene_desc* desc, const bdpt_scene_textures* textures, bdpt_scene** out) {
    if (!desc || !out) return fail(BDPT_ERR_INVALID, "null argument");
    auto s = std::make_unique<bdpt_scene>();
    std::string err;
    if (!load_desc_scene(*desc, textures, s->host, err)) return fail(BDPT_ERR_INVALID, err);
    if (!build_device_layout(s->host, s->layout, err)) return fail(BDPT_ERR_INVALID, err);
    *out = s.release();
    return BDPT_OK;
}

int bdpt_scene_create(const bdpt_scene_desc* desc, bdpt_scene** out) {
    return bdpt_scene_create_textured(desc, nullptr, out);
}

int bdpt_scene_export_textures(const bdpt_scene* s, int32_t array, void* dst, int64_t* bytes, int64_t info[3]) {
    if (!s || !bytes) return fail(BDPT_ERR_INVALID, "null argument");
    const DeviceLayout& L = s->layout;
    const void* src = nullptr;
    size_t n = 0;
    switch (array) {
        case 0: src = L.tex_tab.data(), n = L.tex_tab.size() * 16; break;
        case 1: src = L.tri_st.data(), n = L.tri_st.size() * 4; break;
        case 2: src = L.mat_tex.data(), n = L.mat_tex.size() * 4; break;
        case 3: src = L.tex_dims.data(), n = L.tex_dims.size() * 4; break;
        default: return fail(BDPT_ERR_INVALID, "unknown texture array");
    }
    if (dst) {
        if (*bytes < static_cast<int64_t>(n)) return fail(BDPT_ERR_INVALID, "destination too small");
        if (n) std::memcpy(dst, src, n);
    }
    *bytes = static_cast<int64_t>(n);
    if (info) {
        info[0] = static_cast<int64_t>(L.tex_dims.size() / 3);
        info[1] = L.textured() ? static_cast<int64_t>(L.tex_tab.size() - 2 * L.bsdfs.size()) : 0;
        info[2] = static_cast<int64_t>(L.tex_tab.size() * 16 + L.tri_st.size() * 4);
    }
    return BDPT_OK;
}

int bdpt_scene_export_layout(const bdpt_scene* s, int32_t array, void* dst, int64_t* bytes) {
    if (!s || !bytes) return fail(BDPT_ERR_INVALID, "null argument");
    const DeviceLayout& L = s->layout;
    const uint32_t roots[4] = {L.root_link, L.wroot_link, static_cast<uint32_t>(L.wmax_stack),
                               static_cast<uint32_t>(L.wdepth)};
    const void* src = nullptr;
    size_t n = 0;
    std::vector<float4_t> tmp4;
    std::vector<BsdfRecord> tmpb;
    switch (array) {
        case 0: src = L.tri.data(), n = L.tri.size() * 16; break;
        // (without the leaf-box words, the array as it has been exported so far; with them:
        // bdpt_scene_export_shade_records)
        case 1: tmp4 = device_shade(L, false), src = tmp4.data(), n = tmp4.size() * 16; break;
        case 2: src = L.nodes.data(), n = L.nodes.size() * 16; break;
        case 3: src = L.wnodes.data(), n = L.wnodes.size() * 16; break;
        case 4: src = L.wtri.data(), n = L.wtri.size() * 16; break;
        case 5: src = L.lbox.data(), n = L.lbox.size() * 16; break;
        case 6: tmpb = device_bsdfs(L.bsdfs, L.mat_tex), src = tmpb.data(), n = tmpb.size() * sizeof(BsdfRecord); break;
        case 7: src = L.emitters.data(), n = L.emitters.size() * sizeof(EmitterRecord); break;
        case 8: tmp4 = device_emit_tri(L), src = tmp4.data(), n = tmp4.size() * 16; break;
        case 9: src = L.emit_cdf.data(), n = L.emit_cdf.size() * 4; break;
        case 10: src = L.shape_emitter.data(), n = L.shape_emitter.size() * 4; break;
        case 11: src = roots, n = sizeof(roots); break;
        case 12: src = L.bsdfs.data(), n = L.bsdfs.size() * sizeof(BsdfRecord); break;
        default: return fail(BDPT_ERR_INVALID, "unknown layout array");
    }
    if (dst) {
        if (*bytes < static_cast<int64_t>(n)) return fail(BDPT_ERR_INVALID, "destination too small");
        if (n) std::memcpy(dst, src, n);
    }
    *bytes = static_cast<int64_t>(n);
    return BDPT_OK;
}

// The device shade records as bdpt_ctx_create uploads them (kShadeStride float4 per triangle),
// the reference leaf box or leaf id of the deferred leaf check included (kShadeBox).
int bdpt_scene_export_shade_records(const bdpt_scene* s, void* dst, int64_t* bytes) {
    if (!s || !bytes) return fail(BDPT_ERR_INVALID, "null argument");
    const std::vector<float4_t> rec = device_shade(s->layout);
    const size_t n = rec.size() * 16;
    if (dst) {
        if (*bytes < static_cast<int64_t>(n)) return fail(BDPT_ERR_INVALID, "destination too small");
        if (n) std::memcpy(dst, rec.data(), n);
    }
    *bytes = static_cast<int64_t>(n);
    return BDPT_OK;
}

int bdpt_scene_free(bdpt_scene* scene) {
    delete scene;
    return BDPT_OK;
}

int bdpt_scene_get_info(const bdpt_scene* s, bdpt_scene_info* out) {
    if (!s || !out) return fail(BDPT_ERR_INVALID, "null argument");
    out->triangles = static_cast<int64_t>(s->host.num_triangles());
    out->bvh_nodes = static_cast<int64_t>(s->host.nodes.size());
    out->shapes = static_cast<int64_t>(s->host.shape_first.size());
    out->materials = static_cast<int64_t>(s->host.materials.size());
    out->emitters = static_cast<int64_t>(s->host.emitters.size());
    out->bvh_max_depth = s->host.max_depth;
    const DeviceLayout& L = s->layout;
    int64_t leaves = 0;
    for (const FlatNode& n : s->host.nodes) leaves += (n.right_offset == 0);
    out->bvh_leaves = leaves;
    out->wide_nodes = static_cast<int64_t>(L.wnodes.size() / 8);
    out->wide_depth = L.wdepth;
    out->wide_max_stack = L.wmax_stack;
    out->wide_leaves = L.wleaves;
    out->triangle_tree = L.tri_tree ? 1 : 0;
    out->device_bytes = static_cast<int64_t>((L.tri.size() + L.shade.size() + L.nodes.size() + L.wnodes.size() +
                                              L.wtri.size() + L.lbox.size() + L.emit_tri.size()) * 16 +
                                             L.bsdfs.size() * sizeof(BsdfRecord) +
                                             L.emitters.size() * sizeof(EmitterRecord) + L.emit_cdf.size() * 4 +
                                             L.shape_emitter.size() * 4);
    return BDPT_OK;
}

int bdpt_scene_emitter_count(const bdpt_scene* s, int32_t* out) {
    if (!s || !out) return fail(BDPT_ERR_INVALID, "null argument");
    *out = static_cast<int32_t>(s->host.emitters.size());
    return BDPT_OK;
}

int bdpt_scene_get_emitter(const bdpt_scene* s, int32_t index, bdpt_emitter_info* out) {
    if (!s || !out) return fail(BDPT_ERR_INVALID, "null argument");
    const HostScene& h = s->host;
    if (index < 0 || static_cast<size_t>(index) >= h.emitters.size())
        return fail(BDPT_ERR_INVALID, "bdpt_scene_get_emitter: index " + std::to_string(index) + " is outside [0, " +
                                          std::to_string(h.emitters.size()) + ")");
    const Emitter& e = h.emitters[static_cast<size_t>(index)];
    out->shape = e.shape;
    // the material of the shape's first face: the one whose emission makes the shape an emitter (scene.cpp)
    out->material = -1;
    if (e.shape >= 0 && static_cast<size_t>(e.shape) < h.shape_first.size() && h.shape_count[e.shape] > 0)
        out->material = h.tri_mat[static_cast<size_t>(h.shape_first[e.shape])];
    out->area = e.area;
    for (int k = 0; k < 3; k++) out->radiance[k] = e.radiance[k];
    return BDPT_OK;
}

int bdpt_scene_export(const bdpt_scene* s, float* tri_f32, int32_t* tri_i32, float* node_f32, uint32_t* node_u32) {
    if (!s) return fail(BDPT_ERR_INVALID, "null scene");
    const HostScene& h = s->host;
    for (size_t i = 0; i < h.num_triangles(); i++) {
        const size_t t = static_cast<size_t>(h.order[i]);
        if (tri_f32) {
            std::memcpy(tri_f32 + 18 * i, &h.pos[9 * t], 9 * sizeof(float));
            std::memcpy(tri_f32 + 18 * i + 9, &h.nrm[9 * t], 9 * sizeof(float));
        }
        if (tri_i32) {
            tri_i32[3 * i] = h.tri_shape[t];
            tri_i32[3 * i + 1] = h.tri_prim[t];
            tri_i32[3 * i + 2] = h.tri_mat[t];
        }
    }
    for (size_t i = 0; i < h.nodes.size(); i++) {
        if (node_f32) {
            std::memcpy(node_f32 + 6 * i, h.nodes[i].bmin, 3 * sizeof(float));
            std::memcpy(node_f32 + 6 * i + 3, h.nodes[i].bmax, 3 * sizeof(float));
        }
        if (node_u32) {
            node_u32[3 * i] = h.nodes[i].start;
            node_u32[3 * i + 1] = h.nodes[i].nprims;
            node_u32[3 * i + 2] = h.nodes[i].right_offset;
        }
    }
    return BDPT_OK;
}

int bdpt_scene_export_traversal(const bdpt_scene* s, float* wnodes, float* wtri, float* lbox, uint32_t* root_link) {
    if (!s) return fail(BDPT_ERR_INVALID, "null scene");
    const DeviceLayout& L = s->layout;
    if (wnodes) std::memcpy(wnodes, L.wnodes.data(), L.wnodes.size() * sizeof(float4_t));
    if (wtri) std::memcpy(wtri, L.wtri.data(), L.wtri.size() * sizeof(float4_t));
    if (lbox) std::memcpy(lbox, L.lbox.data(), L.lbox.size() * sizeof(float4_t));
    if (root_link) *root_link = L.wroot_link;
    return BDPT_OK;
}

int bdpt_camera_constants(const bdpt_camera* cam, int32_t width, int32_t height, float out[72]) {
    if (!cam || !out || width <= 0 || height <= 0) return fail(BDPT_ERR_INVALID, "bad camera arguments");
    CameraConstants c;
    camera_constants(cam->eye, cam->at, cam->up, cam->fov, width, height, c);
    std::memcpy(out, &c, sizeof(c));
    return BDPT_OK;
}

int bdpt_device_count(int32_t* count) {
    if (!count) return fail(BDPT_ERR_INVALID, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return BDPT_OK;
}

int bdpt_ctx_destroy(bdpt_ctx* c) {
    if (!c) return BDPT_OK;
    (void)hipSetDevice(c->device);
    // Teardown is best effort: errors here cannot be acted on by the caller.
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
    return BDPT_OK;
}

int bdpt_ctx_create(const bdpt_scene* s, int32_t hip_device, bdpt_ctx** out) {
    if (!s || !out) return fail(BDPT_ERR_INVALID, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(BDPT_ERR_NO_DEVICE, "no HIP device available");
    if (hip_device < 0 || hip_device >= n) return fail(BDPT_ERR_INVALID, "hip_device out of range");
    auto c = std::make_unique<bdpt_ctx>();
    c->device = hip_device;
    HIP_TRY(hipSetDevice(hip_device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, hip_device));
    c->cus = prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    HIP_TRY(hipEventCreateWithFlags(&c->last_use, hipEventDisableTiming));
    const DeviceLayout& L = s->layout;
    int rc;
    if ((rc = upload(c.get(), L.tri.data(), L.tri.size() * 16, c->sc.tri))) return rc;
    if (s->host.shape_first.size() >= (size_t(1) << 24))
        return fail(BDPT_ERR_UNSUPPORTED, "more than 2^24 shapes (the shading record packs the shape id in 24 bits)");
    c->ntri = static_cast<int64_t>(L.shade.size() / 5);
    {  // the device shade records (bdpt_types.h kShadeStride): the host five + v0, one line each
        const std::vector<float4_t> dev_shade = device_shade(L);
        if ((rc = upload(c.get(), dev_shade.data(), dev_shade.size() * 16, c->sc.shade))) return rc;
    }
    if ((rc = upload(c.get(), L.nodes.data(), L.nodes.size() * 16, c->sc.nodes))) return rc;
    if ((rc = upload(c.get(), L.wnodes.data(), L.wnodes.size() * 16, c->sc.wnodes))) return rc;
    c->sc.wroot_link = L.wroot_link;
    c->sc.qnodes = nullptr;
    c->sc.q_ok = 0u;
    if (L.q_ok) {
        if ((rc = upload(c.get(), L.qnodes.data(), L.qnodes.size() * 16, c->sc.qnodes))) return rc;
        c->sc.q_ok = 1u;
    }
    if ((rc = upload(c.get(), L.wtri.data(), L.wtri.size() * 16, c->sc.wtri))) return rc;
    if ((rc = upload(c.get(), L.lbox.data(), L.lbox.size() * 16, c->sc.lbox))) return rc;
    {
        const std::vector<BsdfRecord> dev_bsdfs = device_bsdfs(L.bsdfs, L.mat_tex);
        if ((rc = upload(c.get(), dev_bsdfs.data(), dev_bsdfs.size() * sizeof(BsdfRecord), c->sc.bsdf))) return rc;
        for (const BsdfRecord& b : dev_bsdfs) {
            c->has_glass = c->has_glass || b.kind == BSDF_GLASS;
            c->has_glossy = c->has_glossy || b.kind == BSDF_MIXTURE || b.kind == BSDF_PHONG;
            c->has_null = c->has_null || b.kind == BSDF_NULL;
        }
    }
    if ((rc = upload(c.get(), L.emitters.data(), L.emitters.size() * sizeof(EmitterRecord), c->sc.emit))) return rc;
    {
        const std::vector<float4_t> dev_etri = device_emit_tri(L);
        if ((rc = upload(c.get(), dev_etri.data(), dev_etri.size() * 16, c->sc.emit_tri))) return rc;
    }
    if ((rc = upload(c.get(), L.emit_cdf.data(), L.emit_cdf.size() * 4, c->sc.emit_cdf))) return rc;
    if ((rc = upload(c.get(), L.shape_emitter.data(), L.shape_emitter.size() * 4, c->sc.shape_emitter))) return rc;
    c->sc.tex_tab = nullptr;
    if (L.textured()) {  // map records + texel pool; the texture coordinates ride in the shade records
        if (kShadeStride < kShadeSt + 2)
            return fail(BDPT_ERR_UNSUPPORTED, "bitmap textures need the wide shade records");
        if ((rc = upload(c.get(), L.tex_tab.data(), L.tex_tab.size() * 16, c->sc.tex_tab))) return rc;
        c->textured = true;
        for (size_t m = 0; m < L.bsdfs.size(); m++) c->mat_textured.push_back(L.mat_tex[2 * m] >= 0 || L.mat_tex[2 * m + 1] >= 0);
    }
    {  // bdpt_render_aov's albedo table, from the records as ingested (bdpt_bsdf_type's kinds)
        std::vector<float4_t> mats(2 * std::max<size_t>(L.bsdfs.size(), 1), float4_t{0.f, 0.f, 0.f, 0.f});
        std::vector<float4_t> no_tex(mats.size());
        for (size_t m = 0; m < L.bsdfs.size(); m++) {
            const BsdfRecord& b = L.bsdfs[m];
            const int32_t mode = b.kind == BSDF_DIFFUSE ? 1 : (b.kind == BSDF_MIXTURE || b.kind == BSDF_PHONG ? 2 : 0);
            float fmode;
            std::memcpy(&fmode, &mode, 4);
            mats[2 * m] = float4_t{b.kd[0], b.kd[1], b.kd[2], fmode};
            mats[2 * m + 1] = float4_t{b.ks[0], b.ks[1], b.ks[2], 0.f};
        }
        std::memset(no_tex.data(), 0xff, no_tex.size() * sizeof(float4_t));  // first texel -1: no map
        HIP_TRY(c->aov_mats.reserve(mats.size() * 16));
        HIP_TRY(hipMemcpy(c->aov_mats, mats.data(), mats.size() * 16, hipMemcpyHostToDevice));
        if (!L.textured()) {
            HIP_TRY(c->aov_no_tex.reserve(no_tex.size() * 16));
            HIP_TRY(hipMemcpy(c->aov_no_tex, no_tex.data(), no_tex.size() * 16, hipMemcpyHostToDevice));
        }
    }
    c->sc.root_link = L.root_link;
    c->sc.node_slack = 1u;  // per render: node_slack_needed
    c->tri_tree = L.tri_tree;
    c->wnode_bytes = static_cast<int64_t>(L.wnodes.size()) * 16;
    for (int a = 0; a < 3; a++) c->box_lo[a] = s->host.nodes[0].bmin[a], c->box_hi[a] = s->host.nodes[0].bmax[a];
    {  // the region whose queries the culled, padded traversal tree serves (DevScene::near_lo/hi)
        double diag2 = 0.0;
        for (int a = 0; a < 3; a++) diag2 += (c->box_hi[a] - c->box_lo[a]) * (c->box_hi[a] - c->box_lo[a]);
        const double grow = 100.0 * std::sqrt(diag2);
        for (int a = 0; a < 3; a++) {
            const double lo = c->box_lo[a] - grow, hi = c->box_hi[a] + grow;
            c->sc.near_lo[a] = std::isfinite(lo) ? static_cast<float>(lo) : -__builtin_inff();
            c->sc.near_hi[a] = std::isfinite(hi) ? static_cast<float>(hi) : __builtin_inff();
        }
    }
    c->sc.mt_ring = nullptr;
    c->sc.mt_ring_stride = 0;
    c->sc.nemit = static_cast<int32_t>(L.emitters.size());
    c->sc.inv_nemit = 1.f / static_cast<float>(c->sc.nemit);  // the device's 1.f / nemit, bit for bit
    c->sc.nbsdf = static_cast<int32_t>(L.bsdfs.size());
    c->sc.nshapes = static_cast<int32_t>(L.shape_emitter.size());
    {  // LDS table layout (dev_scene.hpp scene_tables_to_lds), 16-byte aligned parts
        auto up4 = [](uint32_t w) { return (w + 3u) & ~3u; };
        constexpr uint32_t kBudget = kLdsBudget;
        const uint32_t nb = static_cast<uint32_t>(L.bsdfs.size() * sizeof(BsdfRecord) / 4);
        const uint32_t ne = static_cast<uint32_t>(L.emitters.size() * sizeof(EmitterRecord) / 4);
        // BSDF records in LDS unless they do not fit with the emitter records (then
        // the frame renders run bdpt_kernels_hbm.hip); BDPT_BSDF_IN_HBM=1 forces
        // HBM (tests of that build on small scenes).
        const char* force = std::getenv("BDPT_BSDF_IN_HBM");
        const bool hbm = (force && *force == '1') || (up4(up4(dev::kLdsHdr + nb) + ne) * 4u > kBudget);
        c->sc.lds_bsdf_off = hbm ? dev::kNoLds : dev::kLdsHdr;
        c->sc.lds_emit_off = hbm ? dev::kLdsHdr : up4(dev::kLdsHdr + nb);
        c->sc.lds_shape_off = up4(c->sc.lds_emit_off + ne);
        c->sc.lds_words = up4(c->sc.lds_shape_off + static_cast<uint32_t>(L.shape_emitter.size()));
        if (c->sc.lds_words * 4u > kBudget) {  // many shapes: their emitter map stays in HBM
            c->sc.lds_words = c->sc.lds_shape_off;
            c->sc.lds_shape_off = dev::kNoLds;
        }
        if (c->sc.lds_words * 4u > kBudget)
            return fail(BDPT_ERR_UNSUPPORTED, "emitter records exceed the 24 KiB LDS budget");
        // Emitter faces + CDFs join the LDS tables when that costs no resident block.
        c->sc.lds_etri_off = c->sc.lds_ecdf_off = dev::kNoLds;
        c->sc.n_etri = static_cast<int32_t>(L.emit_tri.size() / 5);
        c->sc.n_ecdf = static_cast<int32_t>(L.emit_cdf.size());
        c->lds_words_base = c->sc.lds_words;
        uint32_t etri, ecdf;
        const uint32_t with = emitter_lds_layout(c->sc, c->lds_words_base, etri, ecdf);
        auto blocks = [&](uint32_t words) {
            const size_t bytes = 4 * static_cast<size_t>(words);
            return (hbm ? frame_build_hbm : frame_build).blocks_per_cu(bytes);
        };
        if (with * 4u <= kBudget && blocks(with) >= blocks(c->sc.lds_words)) {
            c->sc.lds_etri_off = etri;
            c->sc.lds_ecdf_off = ecdf;
            c->sc.lds_words = with;
        }
    }
    c->max_depth = s->host.max_depth;
    HIP_TRY(c->work.reserve(sizeof(unsigned long long)));
    HIP_TRY(c->counters.reserve(sizeof(unsigned long long) * kCounterWords));
    HIP_TRY(c->diag.reserve(sizeof(unsigned long long) * dev::kDiagWords));
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0)
            c->wall_khz = khz;
    }
    HIP_TRY(c->sample_out.reserve(16 * sizeof(float)));
    HIP_TRY(c->capped.reserve(sizeof(uint32_t)));
    HIP_TRY(hipMemset(c->capped, 0, sizeof(uint32_t)));
    HIP_TRY(c->dparams.reserve(frame_build.params_bytes));
    // Persistent grid: exactly the resident blocks (no co-residency is assumed:
    // the work queue has no inter-block waits, extra blocks would just queue).
    const size_t dyn = 4 * static_cast<size_t>(c->sc.lds_words);
    c->grid = c->cus * (c->sc.lds_bsdf_off == dev::kNoLds ? frame_build_hbm : frame_build).blocks_per_cu(dyn);
    c->nslots = static_cast<uint32_t>(c->grid * frame_build.block);
    // BDPT_GRID_BLOCKS=n (debugging knob): at most n blocks per frame-kernel launch; the slots
    // stay allocated for the whole grid. With few blocks a small frame gives each wave many
    // chunks, which is what reuses its eye slots (tests/test_gpu_sample_window.py).
    if (const char* gb = debug_knob("BDPT_GRID_BLOCKS")) {
        const int n = std::atoi(gb);
        if (n >= 1) c->grid = std::min(c->grid, n);
    }
    // Traversal stack: worst case of either tree (binary: depth + 1 pending
    // right children; 4-wide: the host-computed bound), the part beyond the
    // kernel's LDS entries in HBM.
    const int depth = std::max(s->host.max_depth + 2, L.wmax_stack + 1);
    const int lds_entries = frame_build.lds_stack;
    c->sc.gdepth = static_cast<uint32_t>(std::max(1, depth - lds_entries));  // per slot (DevScene::gdepth)
    const size_t spill_mega = static_cast<size_t>(c->sc.gdepth) * c->nslots;
    HIP_TRY(c->gstack.reserve(sizeof(uint2) * std::max<size_t>(1, spill_mega)));
    // shadow-ray task rings: their capacity here, their memory in ensure_tasks
    c->task_cap = kTaskCap;
    if (const char* e = std::getenv("BDPT_TASK_CAP")) {  // (sweeps) a power of two in [64, 4096]
        const int v = std::atoi(e);
        if (v >= 64 && v <= 4096 && (v & (v - 1)) == 0) c->task_cap = static_cast<uint32_t>(v);
    }
    *out = c.release();
    return BDPT_OK;
}

// The frame shape, for every frame entry (BDPT, path, direct, feature buffers). Two parts:
// each entry reports a bad size first and a bad shard of rows after its own checks (BDPT,
// feature buffers) or before them (path, direct), as it always has.
static int check_frame_size(const bdpt_frame_params* p) {
    if (!p) return fail(BDPT_ERR_INVALID, "null params");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0) return fail(BDPT_ERR_INVALID, "width/height/spp must be > 0");
    if (static_cast<int64_t>(p->width) * p->height >= (1ll << 31))
        return fail(BDPT_ERR_INVALID, "image too large (W*H must fit int32, as in the reference)");
    return BDPT_OK;
}
static int check_row_shard(const bdpt_frame_params* p) {
    if (p->row_stride < 1 || p->row_offset < 0) return fail(BDPT_ERR_INVALID, "bad row shard");
    return BDPT_OK;
}

static int check_params(const bdpt_frame_params* p) {
    if (int rc = check_frame_size(p)) return rc;
    if (p->rr_depth < 1 || p->rr_depth > kMaxRrDepth)
        return fail(BDPT_ERR_UNSUPPORTED, "rr_depth must be in [1, 1024]");
    if (p->flags & ~(BDPT_FLAG_COUNT | BDPT_FLAG_FULL_TRAVERSAL))
        return fail(BDPT_ERR_UNSUPPORTED, "unknown flag (bit 2, the round-1 wavefront schedule, was removed)");
    if (p->strategy < 0 || p->strategy > 2) return fail(BDPT_ERR_INVALID, "unknown strategy");
    if (int rc = check_row_shard(p)) return rc;
    if (p->russian_roulette != BDPT_RR_NONE && p->russian_roulette != BDPT_RR_LUMINANCE)
        return fail(BDPT_ERR_INVALID, "unknown russian_roulette mode");
    return BDPT_OK;
}

// A sample window (bdpt_render_window) of a frame whose spp the entry has accepted
// (> 0); null = the whole range.
static int check_window(const bdpt_frame_params* p, const bdpt_sample_window* w) {
    if (!w) return BDPT_OK;
    if (w->first < 0) return fail(BDPT_ERR_INVALID, "sample window: first must be >= 0");
    if (w->stride < 1) return fail(BDPT_ERR_INVALID, "sample window: stride must be >= 1");
    if (w->count < 0) return fail(BDPT_ERR_INVALID, "sample window: count must be >= 0");
    if (w->count > 0 && static_cast<int64_t>(w->first) + static_cast<int64_t>(w->count - 1) * w->stride >= p->spp)
        return fail(BDPT_ERR_INVALID, "sample window: count reaches past spp (first + (count - 1) * stride must be < spp = " +
                                          std::to_string(p->spp) + ")");
    return BDPT_OK;
}

constexpr int kExpressDepth = 512;  // Russian roulette: express mode past this many bounces
static dev::DevFrame make_frame(const bdpt_frame_params* p, const bdpt_sample_window* w = nullptr) {
    dev::DevFrame fr{};
    camera_constants(p->camera.eye, p->camera.at, p->camera.up, p->camera.fov, p->width, p->height, fr.cam);
    for (int i = 0; i < 3; i++) fr.cam_o[i] = p->camera.eye[i];
    fr.W = p->width, fr.H = p->height, fr.spp = p->spp, fr.rr_depth = p->rr_depth, fr.strategy = p->strategy;
    fr.seed_base = p->seed_base;
    fr.row_offset = p->row_offset, fr.row_stride = p->row_stride;
    fr.nrows = p->row_offset >= p->height ? 0 : (p->height - p->row_offset + p->row_stride - 1) / p->row_stride;
    fr.flags = p->flags;
    fr.win_first = w ? w->first : 0, fr.win_stride = w ? w->stride : 1, fr.win_count = w ? w->count : p->spp;
    fr.total_samples = static_cast<uint64_t>(fr.nrows) * static_cast<uint64_t>(p->width) * fr.win_count;
    fr.rr_mode = p->russian_roulette == BDPT_RR_LUMINANCE ? 1 : 0;
    fr.depth_cap = fr.rr_mode ? kRrDepthGuard : p->rr_depth;
    fr.lv_max = fr.rr_mode ? std::max(kRrLightVerts, p->rr_depth - 1) : std::max(p->rr_depth - 1, 1);
    fr.inv_spp = 1.f / static_cast<float>(fr.spp);  // IEEE divisions: the bits of the device's rcp_cr
    fr.inv_pixels = 1.f / static_cast<float>(fr.W * fr.H);
    fr.capped = nullptr;  // the context's word, set by the caller
    fr.diag = nullptr;    // the context's timeline, set by bdpt_render
    // Russian-roulette schedule (bdpt_kernels.hip express mode): BDPT_EXPRESS_DEPTH and
    // BDPT_COOP_GROUPS=0 override the build's depth and grouped walks (tests reach the
    // grouped and turn-taking walks on small frames this way; the results are the same)
    fr.express_depth = kExpressDepth;
    if (const char* e = std::getenv("BDPT_EXPRESS_DEPTH")) fr.express_depth = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("BDPT_COOP_GROUPS")) fr.sched_flags |= *e == '0' ? dev::kSchedNoCoopGroups : 0u;
    // BDPT_LEAF_RECHECK=1 (a debugging knob): the deferred reference-leaf check of the frame kernels
    // fails for every closest hit, so each is walked again with the check in the leaf step — the
    // same frame through the path a real failure takes (tests/test_gpu_leaf_defer.py)
    if (leaf_recheck_knob()) fr.sched_flags |= dev::kSchedLeafRecheck;
    return fr;
}

static int ensure_lv(bdpt_ctx* c, int lv_max, uint32_t nslots) {
    const int fields = (c->textured ? frame_build_tex : frame_build).light_vertex_fields;
    HIP_TRY(c->lv.reserve(static_cast<size_t>(std::max(lv_max, 1)) * fields * nslots * sizeof(float)));
    return BDPT_OK;
}

// Shadow-ray task rings, one per wave of the persistent grid (4096 waves x 256 x 40 B = 42 MB
// on 256 CUs). Only the frame kernels without Russian roulette (BDPT_HELP builds) use them,
// so the first render that launches one allocates them; the context's destruction frees them.
static int ensure_tasks(bdpt_ctx* c) {
    HIP_TRY(c->tasks.reserve(static_cast<size_t>(dev::kTaskBytes) * c->task_cap * (c->nslots / 64)));
    return BDPT_OK;
}

// What a scene with bitmap textures does not run: never a wrong image.
static int textured_unsupported(const bdpt_ctx* c, const char* what) {
    if (!c->textured) return BDPT_OK;
    return fail(BDPT_ERR_UNSUPPORTED, std::string("a scene with bitmap textures (map_Kd / map_Ks) does not run ") + what);
}
static int textured_frame_check(const bdpt_ctx* c, const bdpt_frame_params* p) {
    if (!c->textured) return BDPT_OK;
    if (p->russian_roulette != BDPT_RR_NONE)
        return textured_unsupported(c, "with russian_roulette = BDPT_RR_LUMINANCE (texture + Russian roulette)");
    if (p->rr_depth > kLazyRrDepth) return textured_unsupported(c, "with rr_depth > 28 (texture + deep rr_depth)");
    if (c->sc.lds_bsdf_off == dev::kNoLds)
        return textured_unsupported(c, "with the BSDF records in HBM (texture + too many materials for the LDS table)");
    return BDPT_OK;
}

// Interior boxes of the triangle traversal tree are padded by kTriBoxPad x the
// scene diagonal (wide_bvh.hpp), so a ray that hits a triangle passes through
// every box above it over a t-interval of at least 2 pad; slab_fast's rounding
// (RN(1/d), three roundings per plane: < 3.6e-7 (|tn| + |tf|)) can only close
// that interval for boxes more than ~280 diagonals away along the ray. Every
// query of a BDPT frame starts inside the scene box or at the camera, so when
// the camera is within 100 diagonals of the scene the plain tn <= tf test is
// conservative and the ambiguity slack is skipped. Other rays
// (bdpt_intersect's, the refleaf tree's unpadded boxes) keep it.
//
// The slack-free walk tests those boxes by one fma per plane (slab_fma), whose
// error also grows with the origin's distance from 0 (2^-24 |o_i| per plane in
// scene units): it skips the slack only while the origins and the scene box
// also lie within kFmaCoordDiags diagonals of 0, where the per-plane error,
// 2^-23 · 101 + 2^-24 · 300 < 3e-5 diagonals, stays below slab_fast's own bound
// at 100 diagonals (3.6e-7 · 202 = 7.3e-5) and far inside the padding.
constexpr double kFmaCoordDiags = 300.0;
static uint32_t node_slack_needed(const bdpt_ctx* c, const float* const* origins, int n) {
    if (!c->tri_tree) return 1u;
    double diag2 = 0.0;
    for (int a = 0; a < 3; a++) diag2 += (c->box_hi[a] - c->box_lo[a]) * (c->box_hi[a] - c->box_lo[a]);
    if (!(diag2 > 0.0) || !std::isfinite(diag2)) return 1u;
    // the slack-free walk addresses the node planes by 32-bit offsets (load_wnode_nf)
    if (c->wnode_bytes >= (int64_t{1} << 32)) return 1u;
    const double coord_max = kFmaCoordDiags * std::sqrt(diag2);
    for (int a = 0; a < 3; a++)
        if (!(std::fabs(c->box_lo[a]) <= coord_max && std::fabs(c->box_hi[a]) <= coord_max)) return 1u;
    for (int k = 0; k < n; k++) {
        double far2 = 0.0;  // squared distance to the farthest corner of the scene box
        for (int a = 0; a < 3; a++) {
            const double o = origins[k][a];
            const double d = std::max(std::fabs(o - c->box_lo[a]), std::fabs(o - c->box_hi[a]));
            far2 += d * d;
            if (!(std::fabs(o) <= coord_max)) return 1u;
        }
        if (!std::isfinite(far2) || far2 > 1.0e4 * diag2) return 1u;
    }
    return 0u;
}

// A material table the BDPT_GLOSSY 0 code serves: diffuse, mirror and glass records only.
static bool ng_table(const bdpt_ctx* c) { return !c->has_glossy && !c->has_null; }

// The frame-kernel build of a render that textured_frame_check and render_bdpt's own
// checks have accepted. The order of the decisions matters (a textured scene with
// rr_depth 2 runs the textured build, not the short-subpath one). Read per render:
// BDPT_RR_CHAIN=0/1 forces the Russian-roulette build without / with the inline chain,
// BDPT_SPLIT_MAX_RR moves the short-subpath threshold (use_split_build), BDPT_NG_BUILD=0
// keeps the full build (=1 asks for the other and is ignored where the table does not
// allow it). BDPT_BSDF_IN_HBM=1 acts earlier, on the table layout bdpt_ctx_create chose.
static const FrameBuild& pick_frame_build(const bdpt_ctx* c, const bdpt_frame_params* p) {
    if (c->textured) return frame_build_tex;
    if (p->russian_roulette == BDPT_RR_LUMINANCE) {
        // scenes with a dielectric can trap a subpath in a chain of delta bounces: the
        // build that runs a lone chain inline (bdpt_kernels_rrc.hip)
        const char* ce = std::getenv("BDPT_RR_CHAIN");
        return (ce ? *ce == '1' : c->has_glass) ? frame_build_rrc : frame_build_rr;
    }
    if (p->rr_depth > kLazyRrDepth) return frame_build_deep;
    if (c->sc.lds_bsdf_off == dev::kNoLds) return frame_build_hbm;
    if (use_split_build(p->rr_depth)) return frame_build_split;
    // a table of diffuse, mirror and glass records only runs the build without the
    // Mixture / Phong lobes (bdpt_kernels_ng.hip: a vertex that is not delta is diffuse
    // there, so a null BSDF keeps the full build too)
    const char* ne = std::getenv("BDPT_NG_BUILD");
    if (ng_table(c) && !(ne && *ne == '0')) return frame_build_ng;
    return frame_build;
}

// A frame kept as several W x H x 3 planes. One row per kind: what its
// entry points are called in messages, what its plane count is called and how large it may be,
// the phrase of "... are not built ..." and the frame-kernel builds that serve it. A new kind is a
// row here, its BDPT_PLANE_PX case and kernel unit, and its entry pair.

struct PlaneKind {
    const char* entry;            // the render entry's name
    const char* count;            // the plane count's name (a shape: the product's)
    int max;                      // the most planes
    const char* phrase;           // "<phrase> are not built <with what>"
    const FrameBuild* build[2];   // the builds, by Planes::weighting (one build: twice)
    bool shaped;                  // an (n_s, n_t) shape with a weighting comes with the call
    bool mapped;                  // a map from emitters to planes comes with the call
    // a crossed kind: count and max are its outer axis, the groups', and each group
    // holds the planes of this kind, whose count's name, limit or shape the inner axis takes
    const PlaneKind* inner;
};
static const PlaneKind kLayerPlanes = {"bdpt_render_layers", "n_layers", kMaxLayers, "path-length layers",
                                       {&frame_build_layers, &frame_build_layers}, false, false, nullptr};
static const PlaneKind kGroupPlanes = {"bdpt_render_light_groups", "n_groups", kMaxGroups, "light groups",
                                       {&frame_build_groups, &frame_build_groups}, false, true, nullptr};
static const PlaneKind kStrategyPlanes = {"bdpt_render_strategies", "n_s * n_t", kMaxStratS * kMaxStratT,
                                          "strategies (per-(s, t) images)",
                                          {&frame_build_strat, &frame_build_strat_unweighted}, true, false, nullptr};
static const PlaneKind kGroupLayerPlanes = {"bdpt_render_group_layers", "n_groups", kMaxGroups, "light groups x layers",
                                            {&frame_build_groups_layers, &frame_build_groups_layers}, false, true,
                                            &kLayerPlanes};
static const PlaneKind kGroupStrategyPlanes = {"bdpt_render_group_strategies", "n_groups", kMaxGroups,
                                               "light groups x strategies",
                                               {&frame_build_groups_strat, &frame_build_groups_strat_unweighted}, true, true,
                                               &kStrategyPlanes};
// bdpt_render_pixels: the strategy build's planes at the fixed shape (1, 2) for a list of pixels
static const PlaneKind kPixelPlanes = {"bdpt_render_pixels", "2 (the splat and eye planes)", 2, "pixel lists",
                                       {&frame_build_pixels, &frame_build_pixels}, true, false, nullptr};
// what bdpt_group_planes_combine takes: the planes of either crossed kind (n_inner up to the larger limit)
static const PlaneKind kAnyInnerPlanes = {nullptr, "n_inner", std::max(kMaxLayers, kMaxStratS * kMaxStratT), "", {}, false, false, nullptr};
static const PlaneKind kCrossedPlanes = {"bdpt_group_planes_combine", "n_groups", kMaxGroups, "", {}, false, true, &kAnyInnerPlanes};
// the name of a kind's whole plane count
static std::string planes_name(const PlaneKind& k) {
    return k.inner ? std::string(k.count) + " * " + k.inner->count : std::string(k.count);
}

static int check_strategy_shape(const std::string& entry, int32_t n_s, int32_t n_t) {
    if (n_s < 1 || n_s > kMaxStratS) return fail(BDPT_ERR_INVALID, entry + "n_s" + in_range(kMaxStratS));
    if (n_t < 1 || n_t > kMaxStratT) return fail(BDPT_ERR_INVALID, entry + "n_t" + in_range(kMaxStratT));
    return BDPT_OK;
}
static bool strategy_shape_ok(int32_t n_s, int32_t n_t) {
    return n_s >= 1 && n_s <= kMaxStratS && n_t >= 1 && n_t <= kMaxStratT;
}

// One call's planes: its kind (null: the plain frame) and what came with the call.
struct Planes {
    const PlaneKind* kind = nullptr;
    int n = 1;                                  // planes along the kind's own axis (a crossed kind: groups)
    const int32_t* group_of_emitter = nullptr;  // mapped kinds: the caller's host map (null: identity)
    int n_s = 0, n_t = 0, weighting = 0;        // shaped kinds: n_s * n_t planes, BDPT_STRATEGIES_*
    int n_inner = 1;                            // crossed kinds: planes per group (n_layers, n_s * n_t)
    const int32_t* pixels = nullptr;            // the pixel-list kind: the DEVICE list and its length (-1: no list)
    int64_t n_pixels = -1;
    bool listed() const { return n_pixels >= 0; }

    // planes in the framebuffer (sized by it only after check_planes has accepted the counts)
    size_t planes() const { return static_cast<size_t>(n) * n_inner; }
    const FrameBuild& build() const { return *kind->build[weighting == BDPT_STRATEGIES_UNWEIGHTED]; }
    // the kind's DevFrame words (emitter_group: the context's table, uploaded for this call); the
    // map's word and the count's or shape's lie in different unions, so a crossed kind sets both
    void fill(dev::DevFrame& fr, const int32_t* emitter_group) const {
        if (kind->mapped) fr.emitter_group = emitter_group;
        if (kind->shaped) fr.strat_shape = n_s << 8 | n_t;  // (shares n_layers' word)
        else if (kind->inner) fr.n_layers = n_inner;
        else if (!kind->mapped) fr.n_layers = n;
    }
};
// (a shape check_planes refuses keeps one plane: nothing is sized by it)
static int strategy_plane_count(int32_t n_s, int32_t n_t) { return strategy_shape_ok(n_s, n_t) ? n_s * n_t : 1; }
static Planes strategy_planes(int32_t n_s, int32_t n_t, int32_t weighting) {
    Planes pl{&kStrategyPlanes, strategy_plane_count(n_s, n_t)};
    pl.n_s = n_s, pl.n_t = n_t, pl.weighting = weighting;
    return pl;
}
static Planes pixel_planes(const int32_t* pixels_dev, int64_t n_pixels) {
    Planes pl{&kPixelPlanes, 2};
    pl.n_s = 1, pl.n_t = 2, pl.weighting = BDPT_STRATEGIES_WEIGHTED;
    pl.pixels = pixels_dev, pl.n_pixels = n_pixels;
    return pl;
}
static Planes group_layer_planes(const int32_t* group_of_emitter, int32_t n_groups, int32_t n_layers) {
    Planes pl{&kGroupLayerPlanes, n_groups, group_of_emitter};
    pl.n_inner = n_layers;
    return pl;
}
static Planes group_strategy_planes(const int32_t* group_of_emitter, int32_t n_groups, int32_t n_s, int32_t n_t,
                                    int32_t weighting) {
    Planes pl{&kGroupStrategyPlanes, n_groups, group_of_emitter};
    pl.n_s = n_s, pl.n_t = n_t, pl.weighting = weighting, pl.n_inner = strategy_plane_count(n_s, n_t);
    return pl;
}

// What the plane builds serve, checked after check_params and before any launch: the kind's
// count or shape, the size, the map, then what no plane build runs.
static int check_planes(const bdpt_ctx* c, const bdpt_frame_params* p, const Planes& pl) {
    const PlaneKind& k = *pl.kind;
    const std::string entry = std::string(k.entry) + ": ";
    // the kind's own axis is a count unless it is the shape; then the shape, or the inner axis's count
    if ((!k.shaped || k.inner) && (pl.n < 1 || pl.n > k.max))
        return fail(BDPT_ERR_INVALID, entry + k.count + in_range(k.max));
    if (k.shaped) {
        if (int rc = check_strategy_shape(entry, pl.n_s, pl.n_t)) return rc;
        if (pl.weighting != BDPT_STRATEGIES_WEIGHTED && pl.weighting != BDPT_STRATEGIES_UNWEIGHTED)
            return fail(BDPT_ERR_INVALID, entry + "weighting must be BDPT_STRATEGIES_WEIGHTED (0) or "
                                                  "BDPT_STRATEGIES_UNWEIGHTED (1)");
    } else if (k.inner && (pl.n_inner < 1 || pl.n_inner > k.inner->max)) {
        return fail(BDPT_ERR_INVALID, entry + k.inner->count + in_range(k.inner->max));
    }
    if (static_cast<int64_t>(pl.planes()) * p->width * p->height >= kMaxPlanePixels)
        return fail(BDPT_ERR_INVALID, entry + planes_name(k) + " * W * H must be " + kBelowPlanePixels +
                                          " (the shadow-ray task record's pixel field)");
    if (k.mapped) {
        const int nemit = c->sc.nemit;
        if (!pl.group_of_emitter && pl.n != nemit)
            return fail(BDPT_ERR_INVALID, entry + "a null group_of_emitter is the identity map and needs " + k.count +
                                              " equal to the emitter count (" + std::to_string(nemit) + "), got " +
                                              std::to_string(pl.n));
        for (int e = 0; pl.group_of_emitter && e < nemit; e++)
            if (pl.group_of_emitter[e] < 0 || pl.group_of_emitter[e] >= pl.n)
                return fail(BDPT_ERR_INVALID, entry + "group_of_emitter[" + std::to_string(e) + "] = " +
                                                  std::to_string(pl.group_of_emitter[e]) + " is outside [0, " + k.count + ")");
    }
    const char* what = p->flags != 0                              ? "with flags (a counting pass or full traversal)"
                       : p->russian_roulette != BDPT_RR_NONE      ? "with Russian roulette"
                       : p->rr_depth > kLazyRrDepth               ? "with rr_depth > 28"
                       : c->textured                              ? "for a scene with bitmap textures"
                       : c->sc.lds_bsdf_off == dev::kNoLds        ? "with the BSDF records in HBM (too many materials "
                                                                    "for the LDS table)"
                                                                  : nullptr;
    if (what) return fail(BDPT_ERR_UNSUPPORTED, std::string(k.phrase) + " are not built " + what);
    return BDPT_OK;
}

// What a pixel-list render refuses beyond check_planes: a list that cannot lie in the image, a row
// shard, a row order (the list's word in DevFrame is the row order's).
static int check_pixel_list(const bdpt_ctx* c, const bdpt_frame_params* p, const Planes& pl) {
    if (!pl.listed()) return BDPT_OK;
    const std::string entry = std::string(pl.kind->entry) + ": ";
    if (pl.n_pixels > static_cast<int64_t>(p->width) * p->height)
        return fail(BDPT_ERR_INVALID, entry + "n_pixels must be in [0, width * height]");
    if (pl.n_pixels > 0 && !pl.pixels) return fail(BDPT_ERR_INVALID, entry + "pixels must not be NULL");
    if (p->row_offset != 0 || p->row_stride != 1)
        return fail(BDPT_ERR_INVALID, entry + "a pixel list takes no row shard (row_offset must be 0, row_stride 1)");
    if (c->row_order_n)
        return fail(BDPT_ERR_INVALID, entry + "a row order is set on the context (bdpt_set_row_order); clear it first");
    return BDPT_OK;
}

// bdpt_render and the BDPT form of bdpt_render_window (w null: every sample); with planes:
// the plane kinds' render entries (fb is pl.planes() planes, the kind's build; check_planes refuses
// what it does not serve).
static int render_bdpt(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, float* fb,
                       void* hip_stream, const Planes& pl = Planes{}) {
    if (!c || !fb) return fail(BDPT_ERR_INVALID, "null argument");
    int rc = check_params(p);
    if (rc) return rc;
    if ((rc = check_window(p, w))) return rc;
    if (pl.kind && (rc = check_planes(c, p, pl))) return rc;
    if ((rc = check_pixel_list(c, p, pl))) return rc;
    if ((rc = textured_frame_check(c, p))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    dev::DevFrame fr = make_frame(p, w);
    if (pl.listed()) {  // the window's samples of the listed pixels (no row order: refused above)
        fr.pixel_list = pl.pixels;
        fr.total_samples = static_cast<uint64_t>(pl.n_pixels) * static_cast<uint64_t>(fr.win_count);
    }
    fr.capped = c->capped;
    if (!fr.rr_mode && fr.total_samples > 0 && (rc = ensure_tasks(c))) return rc;
    fr.tasks = c->tasks;
    fr.task_cap = c->task_cap;
    if (c->row_order_n) {
        if (c->row_order_n != fr.nrows)
            return fail(BDPT_ERR_INVALID, "the row order set by bdpt_set_row_order has " + std::to_string(c->row_order_n) +
                                              " rows, the shard " + std::to_string(fr.nrows));
        fr.row_order = c->row_order;
    }
    const bool hbm = c->sc.lds_bsdf_off == dev::kNoLds;
    const bool rr = fr.rr_mode != 0;
    const float* eye[1] = {p->camera.eye};
    if (hbm && (p->rr_depth > kLazyRrDepth || rr))
        return fail(BDPT_ERR_UNSUPPORTED, "rr_depth > 28 or Russian roulette with BSDF records in HBM (too many "
                                          "materials for the LDS table) is not built");
    if ((rc = ensure_lv(c, fr.lv_max, c->nslots))) return rc;
    // Shading threshold of the frame kernels: a scene whose tree is deep (from
    // kDeepSceneTris triangles: longer walks) shades at 36 ready lanes, others at 44
    // (round 5, r5m / r5ag: synth1m 1024^2x64 191.8 vs 188.5 Msamples/s at 40 / 44,
    // then 205.6 / 205.1 / 205.2 at 36 vs 203.8 / 203.3 / 204.6 at 40; Caustic and
    // HardLight 0.3-0.8 % slower below 44). BDPT_SHADE_READY overrides it (sweeps).
    fr.shade_ready = c->ntri >= kDeepSceneTris ? 36 : 44;
    if (const char* e = std::getenv("BDPT_SHADE_READY")) fr.shade_ready = std::max(1, std::min(64, std::atoi(e)));
    dev::DevScene sc = c->sc;
    sc.node_slack = node_slack_needed(c, eye, 1);
    if (p->rr_depth > kLazyRrDepth || rr) {  // draws past 226: the lanes' MT19937 rings
        HIP_TRY(c->mt_ring.reserve(sizeof(uint32_t) * kMtRingSlotWords * static_cast<size_t>(c->nslots)));
        sc.mt_ring = c->mt_ring;
        sc.mt_ring_stride = 1;  // slot-major blocks of kMtRingSlotWords words (DevScene::mt_ring)
    }
    if ((rc = begin_use(c, st))) return rc;
    if (pl.kind && pl.kind->mapped) {  // the call's table, from the context's own host copy, in stream order
        const size_t nemit = static_cast<size_t>(c->sc.nemit);
        c->emitter_group_host.resize(nemit);
        for (size_t e = 0; e < nemit; e++)
            c->emitter_group_host[e] = pl.group_of_emitter ? pl.group_of_emitter[e] : static_cast<int32_t>(e);
        HIP_TRY(c->emitter_group.reserve(std::max<size_t>(nemit * sizeof(int32_t), 16)));
        HIP_TRY(hipMemcpyAsync(c->emitter_group, c->emitter_group_host.data(), nemit * sizeof(int32_t),
                               hipMemcpyHostToDevice, st));
    }
    if (pl.kind) pl.fill(fr, c->emitter_group);
    HIP_TRY(hipMemsetAsync(c->work, 0, sizeof(unsigned long long), st));
    // BDPT_SAMPLE_RANGE="lo,hi" (debugging aid, tools/rr_find.py): only the shard's
    // samples [lo, hi) — the work counter starts at lo and the frame ends at hi
    uint64_t range_lo = 0;  // samples [range_lo, total_samples) are rendered
    if (const char* sr = debug_knob("BDPT_SAMPLE_RANGE")) {
        unsigned long long lo = 0, hi = 0;
        if (std::sscanf(sr, "%llu,%llu", &lo, &hi) == 2 && lo <= hi) {
            fr.total_samples = std::min<uint64_t>(fr.total_samples, hi);
            c->work_init = std::min<unsigned long long>(lo, fr.total_samples);
            range_lo = c->work_init;
            HIP_TRY(hipMemcpyAsync(c->work, &c->work_init, sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        }
    }
    if ((p->flags & BDPT_FLAG_COUNT) && fr.nrows > 0) {  // queries per local row (bdpt_get_row_costs)
        HIP_TRY(c->row_cost.reserve(sizeof(unsigned long long) * fr.nrows));
        HIP_TRY(hipMemsetAsync(c->row_cost, 0, sizeof(unsigned long long) * fr.nrows, st));
        fr.row_cost = c->row_cost;
        c->row_cost_n = fr.nrows;
    }
    HIP_TRY(hipMemsetAsync(c->diag, 0, sizeof(unsigned long long) * dev::kDiagWords, st));
    HIP_TRY(hipMemsetAsync(c->diag + dev::kDiagStart, 0xff, sizeof(unsigned long long), st));
    fr.diag = c->diag;
    if ((rc = begin_timed(c, st))) return rc;
    int64_t launches = 0;
    if (fr.total_samples > 0) {
        const FrameBuild& b = pl.kind ? pl.build() : pick_frame_build(c, p);
        c->last_kernel_glossy = 1;  // (until the launches below have succeeded)
        // Never more resident blocks than the slots allocated. c->grid is the default build's
        // blocks_per_cu of these LDS bytes (the HBM build's on an HBM table; bdpt_ctx_create),
        // so for those two builds the clamp changes nothing.
        const int grid = std::min(c->grid, c->cus * b.blocks_per_cu(4 * static_cast<size_t>(c->sc.lds_words)));
        // the Russian-roulette builds' continuation pass (park_depth_setting)
        const int park_depth = b.launch_chain ? park_depth_setting() : 0;
        const bool park = park_depth > 0 && !(p->flags & BDPT_FLAG_COUNT);
        if (park) {
            const size_t words = static_cast<size_t>(c->nslots) * (kParkSlotWords + 1) + 1;
            HIP_TRY(c->park.reserve(words * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(c->park, 0, words * sizeof(uint32_t), st));
            fr.park = c->park;
            fr.park_depth = park_depth;
            fr.park_flags = dev::kParkOn;
        }
        HIP_TRY(b.launch_frame(sc, fr, fb, c->lv, c->gstack, c->nslots, c->work, c->counters, grid, st, c->dparams));
        const int rounds = park ? park_rounds_setting() : 0;
        for (int k = 0; k < rounds; k++) {
            HIP_TRY(b.launch_chain(sc, fr, fb, c->lv, c->gstack, c->nslots, c->work, c->counters, kChainGrid, st,
                                   c->dparams));
            uint32_t* const list = c->park + static_cast<size_t>(c->nslots) * kParkSlotWords;
            HIP_TRY(hipMemsetAsync(list, 0, sizeof(uint32_t), st));  // the resume launch parks anew
            dev::DevFrame fres = fr;
            fres.park_flags = dev::kParkResume | (k + 1 < rounds ? dev::kParkOn : 0u);
            HIP_TRY(b.launch_frame(sc, fres, fb, c->lv, c->gstack, c->nslots, c->work, c->counters, grid, st,
                                   c->dparams));
        }
        c->last_kernel = b.name;
        c->last_kernel_glossy = b.glossy;
        launches += 1 + 2 * rounds;
    }
    return end_timed(c, st, static_cast<int64_t>(fr.total_samples - range_lo), launches, true);
}

int bdpt_render(bdpt_ctx* c, const bdpt_frame_params* p, float* fb, void* hip_stream) {
    return render_bdpt(c, p, nullptr, fb, hip_stream);
}

int bdpt_render_layers(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, int32_t n_layers,
                       float* fb_layers, void* hip_stream) {
    return render_bdpt(c, p, w, fb_layers, hip_stream, Planes{&kLayerPlanes, n_layers});
}

int bdpt_render_light_groups(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, int32_t n_groups,
                             const int32_t* group_of_emitter, float* fb_groups, void* hip_stream) {
    return render_bdpt(c, p, w, fb_groups, hip_stream, Planes{&kGroupPlanes, n_groups, group_of_emitter});
}

int bdpt_render_strategies(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, int32_t n_s, int32_t n_t,
                           int32_t weighting, float* fb_planes, void* hip_stream) {
    return render_bdpt(c, p, w, fb_planes, hip_stream, strategy_planes(n_s, n_t, weighting));
}

int bdpt_render_group_layers(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                             const int32_t* group_of_emitter, int32_t n_groups, int32_t n_layers, float* fb_planes,
                             void* hip_stream) {
    return render_bdpt(c, p, w, fb_planes, hip_stream, group_layer_planes(group_of_emitter, n_groups, n_layers));
}

int bdpt_render_group_strategies(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                                 const int32_t* group_of_emitter, int32_t n_groups, int32_t n_s, int32_t n_t,
                                 int32_t weighting, float* fb_planes, void* hip_stream) {
    return render_bdpt(c, p, w, fb_planes, hip_stream,
                       group_strategy_planes(group_of_emitter, n_groups, n_s, n_t, weighting));
}

int bdpt_strategies_shape(int32_t rr_depth, int32_t strategy, int32_t* n_s, int32_t* n_t) {
    if (!n_s || !n_t) return fail(BDPT_ERR_INVALID, "null argument");
    if (rr_depth < 1 || rr_depth > kLazyRrDepth)
        return fail(BDPT_ERR_INVALID, "bdpt_strategies_shape: rr_depth must be in [1, 28]");
    if (strategy < BDPT_STRATEGY_BDPT || strategy > BDPT_STRATEGY_PATH_TRACING)
        return fail(BDPT_ERR_INVALID, "bdpt_strategies_shape: strategy must be a BDPT_STRATEGY_* value");
    // s reaches D through a light vertex stored at depth D - 1, t through an eye vertex at depth
    // D - 1; light tracing's primary emission is (0, 2) whatever D is. One shape for the three
    // strategies: the planes of a frame's light- and path-tracing forms line up with its BDPT form's.
    *n_s = std::max(rr_depth, 1) + 1;
    *n_t = std::max(rr_depth, 2);
    return BDPT_OK;
}

// What the three combine entries check alike.
static int check_gains_finite(const char* entry, const float* gains, int planes) {
    for (int i = 0; gains && i < 3 * planes; i++)
        if (!std::isfinite(gains[i]))
            return fail(BDPT_ERR_INVALID, std::string(entry) + ": gains[" + std::to_string(i / 3) + "][" +
                                              std::to_string(i % 3) + "] is not finite");
    return BDPT_OK;
}
static bool overlap(const float* a, size_t a_floats, const float* b, size_t b_floats) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pb < pa + a_floats * sizeof(float) && pa < pb + b_floats * sizeof(float);
}
// n planes of kind k (its count's name and limit; a crossed kind: n groups of n_inner planes)
// combined into one width x height frame
static int check_combine_shape(const char* entry, const PlaneKind& k, int32_t n, int32_t width, int32_t height,
                               int32_t n_inner = 1) {
    if (n < 1 || n > k.max) return fail(BDPT_ERR_INVALID, std::string(entry) + ": " + k.count + in_range(k.max));
    if (k.inner && (n_inner < 1 || n_inner > k.inner->max))
        return fail(BDPT_ERR_INVALID, std::string(entry) + ": " + k.inner->count + in_range(k.inner->max));
    if (width <= 0 || height <= 0 || static_cast<int64_t>(n) * n_inner * width * height >= kMaxPlanePixels)
        return fail(BDPT_ERR_INVALID, std::string(entry) + ": width/height must be > 0 and " + planes_name(k) +
                                          " * W * H " + kBelowPlanePixels);
    return BDPT_OK;
}

int bdpt_strategies_sheet(bdpt_ctx* c, const float* planes, int32_t n_s, int32_t n_t, int32_t width, int32_t height,
                          const float* gains, float* out, void* hip_stream) {
    const char* const entry = "bdpt_strategies_sheet";
    if (!c || !planes || !out) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_strategy_shape(std::string(entry) + ": ", n_s, n_t)) return rc;
    if (width <= 0 || height <= 0) return fail(BDPT_ERR_INVALID, std::string(entry) + ": width/height must be > 0");
    const int64_t floats = static_cast<int64_t>(n_s) * n_t * width * height * 3;  // the planes' and the sheet's size alike
    if (floats >= (int64_t{1} << 31))
        return fail(BDPT_ERR_INVALID, std::string(entry) + ": the sheet (n_s * n_t * W * H * 3 floats) must be below 2^31 floats");
    if (int rc = check_gains_finite(entry, gains, n_s * n_t)) return rc;
    if (overlap(planes, floats, out, floats)) return fail(BDPT_ERR_INVALID, std::string(entry) + ": out overlaps the planes");
    return combine_planes(c, hip_stream, gains, 3 * n_s * n_t, [&](const float* dgains, hipStream_t st) {
        return launch_strategies_sheet(planes, n_s, n_t, width, height, dgains, out, st);
    });
}

int bdpt_light_groups_relight(bdpt_ctx* c, const float* fb_groups, int32_t n_groups, int32_t width, int32_t height,
                              const float* gains, float* out, void* hip_stream) {
    const char* const entry = "bdpt_light_groups_relight";
    if (!c || !fb_groups || !gains || !out) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_combine_shape(entry, kGroupPlanes, n_groups, width, height)) return rc;
    if (int rc = check_gains_finite(entry, gains, n_groups)) return rc;
    const size_t n = static_cast<size_t>(width) * height * 3;
    if (overlap(fb_groups, n * n_groups, out, n)) return fail(BDPT_ERR_INVALID, std::string(entry) + ": out overlaps the planes");
    return combine_planes(c, hip_stream, nullptr, 0, [&](const float*, hipStream_t st) {  // (the gains are a kernel argument)
        return launch_relight(fb_groups, n, n_groups, gains, out, st);
    });
}

int bdpt_group_planes_combine(bdpt_ctx* c, const float* planes, int32_t n_groups, int32_t n_inner, int32_t width,
                              int32_t height, const float* gains, const float* weights, float* out, void* hip_stream) {
    const char* const entry = kCrossedPlanes.entry;
    if (!c || !planes || !out) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_combine_shape(entry, kCrossedPlanes, n_groups, width, height, n_inner)) return rc;
    if (int rc = check_gains_finite(entry, gains, n_groups)) return rc;
    for (int j = 0; weights && j < n_inner; j++)
        if (!std::isfinite(weights[j]))
            return fail(BDPT_ERR_INVALID, std::string(entry) + ": weights[" + std::to_string(j) + "] is not finite");
    const size_t n = static_cast<size_t>(width) * height * 3;
    if (overlap(planes, n * n_groups * n_inner, out, n))
        return fail(BDPT_ERR_INVALID, std::string(entry) + ": out overlaps the planes");
    // null gains and weights are ones: the kernel multiplies by them like any other (x * 1 is x)
    const std::vector<float> ones(std::max<size_t>(3 * static_cast<size_t>(n_groups), n_inner), 1.f);
    const float* const g = gains ? gains : ones.data();
    return combine_planes(c, hip_stream, weights ? weights : ones.data(), n_inner, [&](const float* dweights, hipStream_t st) {
        return launch_group_planes_combine(planes, n, n_groups, n_inner, g, dweights, out, st);
    });
}

int bdpt_layers_compose(bdpt_ctx* c, const float* fb_layers, int32_t n_layers, int32_t width, int32_t height,
                        uint64_t mask, float* out, void* hip_stream) {
    const char* const entry = "bdpt_layers_compose";
    if (!c || !fb_layers || !out) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_combine_shape(entry, kLayerPlanes, n_layers, width, height)) return rc;
    if (mask == 0) return fail(BDPT_ERR_INVALID, std::string(entry) + ": empty layer mask");
    if (n_layers < kMaxLayers && (mask >> n_layers) != 0)
        return fail(BDPT_ERR_INVALID, std::string(entry) + ": the mask has bits at or above n_layers");
    return combine_planes(c, hip_stream, nullptr, 0, [&](const float*, hipStream_t st) {
        return launch_layers_compose(fb_layers, static_cast<size_t>(width) * height * 3, mask, out, st);
    });
}

// PathTracerIntegrator (path.h) on the same substrate: pt_kernels.hip.
constexpr int kPtMaxLevels = 512;  // recursion levels per lane under Russian roulette (P(> 512) ~ 0.95^507)

// The path / direct frame kernels read the BSDF records from the LDS table only.
static int pt_frame_tables(const bdpt_ctx* c) {
    if (c->sc.lds_bsdf_off == dev::kNoLds)
        return fail(BDPT_ERR_UNSUPPORTED, "the path / direct frame renders need the BSDF records in the LDS table "
                                          "(too many materials; bdpt_render and the single-sample calls take them)");
    return BDPT_OK;
}

static int ensure_pt(bdpt_ctx* c, int levels) {
    if (!c->pt_nslots) {
        // Up to 4 resident 256-lane blocks per CU (4 waves/SIMD at 128 VGPRs;
        // measured 70 -> 119 Msamples/s from 2), within the BDPT grid (the
        // traversal-stack overflow buffer is sized for that many slots).
        // BDPT_PT_BLOCKS overrides the cap (experiments). Level stacks: 512 x 80 B
        // per slot, ~10.7 GB at 256 CUs x 1024 slots under Russian roulette.
        const char* cap_env = std::getenv("BDPT_PT_BLOCKS");
        const int cap = cap_env ? std::max(1, std::atoi(cap_env)) : 4;
        c->pt_grid = std::min(c->grid, c->cus * std::min(cap, pt_blocks_per_cu(4 * static_cast<size_t>(c->sc.lds_words))));
        c->pt_nslots = static_cast<uint32_t>(c->pt_grid) * 256u;
    }
    HIP_TRY(c->pt_dparams.reserve(pt_params_bytes()));
    HIP_TRY(c->pt_ring.reserve(sizeof(uint32_t) * 624 * static_cast<size_t>(c->pt_nslots)));
    HIP_TRY(c->pt_levels.reserve(sizeof(float4) * 5 * static_cast<size_t>(levels) * c->pt_nslots));
    return BDPT_OK;
}

// The path tracer's and direct integrator's scene: its queries start inside the
// scene box or at the camera, as the BDPT frame's do, so the same per-render
// choice of interior-box test applies (node_slack_needed).
#ifndef BDPT_PT_SLACK_FREE
#define BDPT_PT_SLACK_FREE 1  // 0: the path tracer keeps the slack test everywhere (A/B only)
#endif
static dev::DevScene pt_scene(const bdpt_ctx* c, const bdpt_frame_params* p) {
    dev::DevScene sc = c->sc;
    const float* eye[1] = {p->camera.eye};
    sc.node_slack = BDPT_PT_SLACK_FREE ? node_slack_needed(c, eye, 1) : 1u;
    return sc;
}

// The launch_pt settings block of a path tracer and the level-stack depth it needs: maxDepth
// levels, or Russian roulette's (check_pt_levels).
static int path_sample_settings(const bdpt_path_params* path, int32_t settings[8], int& levels) {
    if (!path) return fail(BDPT_ERR_INVALID, "null argument");
    if (path->emitter_samples < 0 || path->bsdf_samples < 0) return fail(BDPT_ERR_INVALID, "negative sample counts");
    const bool rr = path->is_explicit && path->max_depth == -1;
    levels = rr ? kPtMaxLevels : std::max(path->max_depth, 0) + 2;
    const int32_t s[8] = {path->is_explicit ? 1 : 0, path->max_depth, path->rr_depth, 0, path->emitter_samples,
                          path->bsdf_samples, levels, 0};
    std::memcpy(settings, s, sizeof(s));
    std::memcpy(&settings[3], &path->rr_prob, 4);
    return BDPT_OK;
}
static int check_pt_levels(int levels) {
    if (levels > kPtMaxLevels) return fail(BDPT_ERR_UNSUPPORTED, "maxDepth > 510 is not supported");
    return BDPT_OK;
}

// DirectIntegrator (direct.h) on the path tracer's kernel: one level, no recursion.
static int direct_sample_settings(const bdpt_direct_params* d, int32_t settings[8]) {
    if (!d) return fail(BDPT_ERR_INVALID, "null argument");
    if (d->sampling_strategy < BDPT_DIRECT_AREA || d->sampling_strategy > BDPT_DIRECT_MIS)
        return fail(BDPT_ERR_INVALID, "Error: wrong strategy");  // direct.h:460
    if (d->emitter_samples < 0 || d->bsdf_samples < 0) return fail(BDPT_ERR_INVALID, "negative sample counts");
    const int32_t s[8] = {1, -1, 0, 0, d->emitter_samples, d->bsdf_samples, 1, d->sampling_strategy};
    std::memcpy(settings, s, sizeof(s));
    return BDPT_OK;
}

// The frame render of the path tracer and of the direct integrator (w null: every sample).
// integrator: the entry's bdpt_path_params / bdpt_direct_params; settings_of(integrator, block,
// levels): its checks and its settings block (path_sample_settings / direct_sample_settings),
// which run where the two entries always ran them, after the row shard's check and before
// the window's; what: how the entry refuses a scene with bitmap textures.
static int render_pt_frame(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, const void* integrator,
                           int (*settings_of)(const void*, int32_t*, int&), const char* what, float* fb,
                           void* hip_stream) {
    if (!c || !fb || !integrator) return fail(BDPT_ERR_INVALID, "null argument");
    int rc, levels = 1;
    int32_t settings[8];
    if ((rc = textured_unsupported(c, what)) || (rc = check_frame_size(p)) || (rc = check_row_shard(p)) ||
        (rc = settings_of(integrator, settings, levels)) || (rc = check_window(p, w)) || (rc = check_pt_levels(levels)))
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = pt_frame_tables(c)) || (rc = ensure_pt(c, levels))) return rc;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const dev::DevFrame fr = make_frame(p, w);
    if ((rc = begin_use(c, st))) return rc;
    HIP_TRY(hipMemsetAsync(c->work, 0, sizeof(unsigned long long), st));
    if ((rc = begin_timed(c, st))) return rc;
    if (fr.total_samples > 0)
        HIP_TRY(launch_pt(pt_scene(c, p), fr, settings, fb, c->pt_levels, c->pt_ring, c->gstack, c->pt_nslots, c->work,
                          c->counters, c->pt_grid, st, c->pt_dparams));
    return end_timed(c, st, static_cast<int64_t>(fr.total_samples), fr.total_samples > 0 ? 1 : 0);
}

static int render_path(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                       const bdpt_path_params* path, float* fb, void* hip_stream) {
    return render_pt_frame(
        c, p, w, path,
        [](const void* path, int32_t* settings, int& levels) {
            return path_sample_settings(static_cast<const bdpt_path_params*>(path), settings, levels);
        },
        "the path integrator (texture + bdpt_render_path)", fb, hip_stream);
}

static int render_direct(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                         const bdpt_direct_params* d, float* fb, void* hip_stream) {
    return render_pt_frame(
        c, p, w, d,
        [](const void* d, int32_t* settings, int&) {
            return direct_sample_settings(static_cast<const bdpt_direct_params*>(d), settings);
        },
        "the direct integrator (texture + bdpt_render_direct)", fb, hip_stream);
}

int bdpt_render_path(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_path_params* path, float* fb,
                     void* hip_stream) {
    return render_path(c, p, nullptr, path, fb, hip_stream);
}

int bdpt_render_direct(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_direct_params* d, float* fb,
                       void* hip_stream) {
    return render_direct(c, p, nullptr, d, fb, hip_stream);
}

// What the path / direct host entries check before they stage the frame.
static int pt_host_args(const bdpt_ctx* c, const bdpt_frame_params* p, const float* fb_host) {
    if (!c || !fb_host || !p) return fail(BDPT_ERR_INVALID, "null argument");
    if (p->width <= 0 || p->height <= 0) return fail(BDPT_ERR_INVALID, "width/height must be > 0");
    return BDPT_OK;
}

static int render_path_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                            const bdpt_path_params* path, float* fb_host) {
    int rc = pt_host_args(c, p, fb_host);
    if (rc) return rc;
    if ((rc = stage_host(c, fb_host, static_cast<size_t>(p->width) * p->height * 3,
                         [&](float* fb) { return render_path(c, p, w, path, fb, c->stream); })))
        return rc;
    bdpt_stats st;
    if ((rc = bdpt_get_stats(c, &st))) return rc;
    if (st.counters[1] != 0)
        return fail(BDPT_ERR_UNSUPPORTED, std::to_string(st.counters[1]) + " samples outgrew the path tracer's level stack");
    return BDPT_OK;
}

static int render_direct_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                              const bdpt_direct_params* d, float* fb_host) {
    if (int rc = pt_host_args(c, p, fb_host)) return rc;
    return stage_host(c, fb_host, static_cast<size_t>(p->width) * p->height * 3,
                      [&](float* fb) { return render_direct(c, p, w, d, fb, c->stream); });
}

int bdpt_render_path_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_path_params* path, float* fb_host) {
    return render_path_host(c, p, nullptr, path, fb_host);
}

int bdpt_render_direct_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_direct_params* d, float* fb_host) {
    return render_direct_host(c, p, nullptr, d, fb_host);
}

static int ensure_sample_buffers(bdpt_ctx* c, int32_t splat_cap) {
    HIP_TRY(c->mt_state.reserve(sizeof(uint32_t) * BDPT_MT19937_WORDS));
    if (splat_cap > c->splat_cap) {
        c->splat_cap = 0;
        HIP_TRY(c->splat_list.reserve(sizeof(float) * 4 * (static_cast<size_t>(splat_cap) + 1)));
        c->splat_cap = splat_cap;
    }
    return BDPT_OK;
}

static int check_mt_state(const uint32_t* state) {
    if (!state) return fail(BDPT_ERR_INVALID, "null sampler state");
    if (state[BDPT_MT19937_WORDS - 1] > 624u) return fail(BDPT_ERR_INVALID, "sampler state position _M_p > 624");
    return BDPT_OK;
}

// One PathTracerIntegrator / DirectIntegrator::render(ray, sampler) call with the
// caller's std::mt19937 state (settings: the launch_pt block; levels: level-stack
// depth it needs).
static int render_pt_sample(bdpt_ctx* c, const bdpt_frame_params* p, const int32_t settings[8], int levels,
                            const float ray[8], uint32_t* state, float Li[3], uint32_t* taken = nullptr) {
    if (!c || !p || !ray || !Li) return fail(BDPT_ERR_INVALID, "null argument");
    int rc;
    if ((rc = textured_unsupported(c, "the path / direct integrators (texture + bdpt_render_path / _direct sample)")))
        return rc;
    if ((rc = check_mt_state(state))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_pt(c, levels))) return rc;
    if ((rc = ensure_sample_buffers(c, 1))) return rc;
    if ((rc = begin_use(c, c->stream))) return rc;
    const dev::DevFrame fr = make_frame(p);
    const dev::Ray r{dev::f3{ray[0], ray[1], ray[2]}, dev::f3{ray[3], ray[4], ray[5]}, ray[6], ray[7]};
    dev::DevScene sc = c->sc;
    sc.mt_ring = c->mt_state;  // the sample kernel's generator state (mt_state_u32)
    HIP_TRY(hipMemcpyAsync(c->mt_state, state, sizeof(uint32_t) * BDPT_MT19937_WORDS, hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * kCounterWords, c->stream));
    HIP_TRY(launch_pt_sample(sc, fr, settings, c->pt_levels, c->pt_ring, c->gstack, r, c->sample_out, c->counters,
                             c->stream, c->pt_dparams));
    float out[4];
    unsigned long long ctr[2];
    HIP_TRY(hipMemcpyAsync(out, c->sample_out, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ctr, c->counters, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(state, c->mt_state, sizeof(uint32_t) * BDPT_MT19937_WORDS, hipMemcpyDeviceToHost,
                           c->stream));
    if ((rc = end_use(c, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ctr[1] != 0) return fail(BDPT_ERR_UNSUPPORTED, "the sample outgrew the path tracer's level stack");
    Li[0] = out[0], Li[1] = out[1], Li[2] = out[2];
    if (taken) std::memcpy(taken, &out[3], 4);
    return BDPT_OK;
}

int bdpt_render_path_sample_mt(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_path_params* path,
                               const float ray[8], uint32_t state[BDPT_MT19937_WORDS], float Li[3]) {
    int32_t settings[8];
    int levels = 0, rc;
    if ((rc = path_sample_settings(path, settings, levels)) || (rc = check_pt_levels(levels))) return rc;
    return render_pt_sample(c, p, settings, levels, ray, state, Li);
}

int bdpt_render_direct_sample_mt(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_direct_params* d,
                                 const float ray[8], uint32_t state[BDPT_MT19937_WORDS], float Li[3]) {
    int32_t settings[8];
    int rc;
    if ((rc = direct_sample_settings(d, settings))) return rc;
    return render_pt_sample(c, p, settings, 1, ray, state, Li);
}

// (seed, draws) sampler: std::mt19937(seed) advanced by *draws outputs.
static int pt_sample_seeded(bdpt_ctx* c, const bdpt_frame_params* p, const int32_t settings[8], int levels,
                            const float ray[8], uint32_t seed, int32_t* draws, float Li[3]) {
    if (!draws) return fail(BDPT_ERR_INVALID, "null argument");
    if (*draws < 0) return fail(BDPT_ERR_INVALID, "negative draw count");
    uint32_t st[BDPT_MT19937_WORDS], used = 0;
    mt19937_state(seed, *draws, st);
    int rc;
    if ((rc = render_pt_sample(c, p, settings, levels, ray, st, Li, &used))) return rc;
    *draws += static_cast<int32_t>(used);
    return BDPT_OK;
}

int bdpt_render_path_sample(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_path_params* path,
                            const float ray[8], uint32_t seed, int32_t* draws, float Li[3]) {
    int32_t settings[8];
    int levels = 0, rc;
    if ((rc = path_sample_settings(path, settings, levels)) || (rc = check_pt_levels(levels))) return rc;
    return pt_sample_seeded(c, p, settings, levels, ray, seed, draws, Li);
}

int bdpt_render_direct_sample(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_direct_params* d,
                              const float ray[8], uint32_t seed, int32_t* draws, float Li[3]) {
    int32_t settings[8];
    int rc;
    if ((rc = direct_sample_settings(d, settings))) return rc;
    return pt_sample_seeded(c, p, settings, 1, ray, seed, draws, Li);
}

int bdpt_debug_math(int32_t device, int32_t fn, const float* x, const float* y, float* out, int64_t n) {
    const bool two = fn == BDPT_MATH_POWF || fn == BDPT_MATH_POW_W || fn == BDPT_MATH_DIV_W;
    if (!x || !out || n < 0 || (two && !y) || fn < 0 || fn > BDPT_MATH_RSQRT_W)
        return fail(BDPT_ERR_INVALID, "bad argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(BDPT_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(BDPT_ERR_INVALID, "bad device");
    HIP_TRY(hipSetDevice(device));
    if (n == 0) return BDPT_OK;
    DevBuf<float> dx, dy, dout;
    const size_t bytes = sizeof(float) * static_cast<size_t>(n);
    hipError_t e = dx.reserve(bytes);
    if (e == hipSuccess) e = dy.reserve(bytes);
    if (e == hipSuccess) e = dout.reserve(bytes);
    if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, y ? y : x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = fn >= BDPT_MATH_POW_W ? launch_math_check_fw(fn, dx, dy, dout, n, nullptr)
                                  : launch_math_check(fn, dx, dy, dout, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(BDPT_ERR_HIP, std::string("bdpt_debug_math: ") + hipGetErrorString(e));
    return BDPT_OK;
}

const char* bdpt_last_kernel(const bdpt_ctx* c) { return c ? c->last_kernel : ""; }
int bdpt_last_kernel_glossy(const bdpt_ctx* c) { return c ? c->last_kernel_glossy : 1; }

int bdpt_set_row_order(bdpt_ctx* c, const int32_t* order, int32_t n) {
    if (!c || n < 0 || (n > 0 && !order)) return fail(BDPT_ERR_INVALID, "bdpt_set_row_order: bad argument");
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int32_t i = 0; i < n; i++) {
        if (order[i] < 0 || order[i] >= n || seen[static_cast<size_t>(order[i])])
            return fail(BDPT_ERR_INVALID, "bdpt_set_row_order: not a permutation of 0..n-1");
        seen[static_cast<size_t>(order[i])] = 1;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // a render in flight may read the previous order
    c->row_order_n = 0;
    if (n == 0) return BDPT_OK;
    HIP_TRY(c->row_order.reserve(sizeof(int32_t) * static_cast<size_t>(n)));
    HIP_TRY(hipMemcpy(c->row_order, order, sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyHostToDevice));
    c->row_order_n = n;
    return BDPT_OK;
}

int bdpt_get_row_costs(bdpt_ctx* c, int64_t* costs, int32_t n) {
    if (!c || !costs) return fail(BDPT_ERR_INVALID, "null argument");
    if (!c->row_cost || n != c->row_cost_n)
        return fail(BDPT_ERR_INVALID, "bdpt_get_row_costs: no counting render of a " + std::to_string(n) + "-row shard");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> h(static_cast<size_t>(n));
    HIP_TRY(hipMemcpy(h.data(), c->row_cost, sizeof(unsigned long long) * static_cast<size_t>(n), hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < n; i++) costs[i] = static_cast<int64_t>(h[static_cast<size_t>(i)]);
    return BDPT_OK;
}

int bdpt_get_stats(bdpt_ctx* c, bdpt_stats* out) {
    if (!c || !out) return fail(BDPT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (c->pending_timing) {
        HIP_TRY(hipEventSynchronize(c->ev1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->stats.kernel_ms = ms;
        unsigned long long host[BDPT_NUM_COUNTERS];
        HIP_TRY(hipMemcpy(host, c->counters, sizeof(host), hipMemcpyDeviceToHost));
        for (int i = 0; i < BDPT_NUM_COUNTERS; i++) c->stats.counters[i] = static_cast<int64_t>(host[i]);
        uint32_t capped = 0;
        HIP_TRY(hipMemcpy(&capped, c->capped, sizeof(capped), hipMemcpyDeviceToHost));
        c->stats.capped_samples = capped;
        unsigned long long mx[3];
        HIP_TRY(hipMemcpy(mx, c->counters + BDPT_NUM_COUNTERS, sizeof(mx), hipMemcpyDeviceToHost));
        c->stats.max_light_depth = static_cast<int64_t>(mx[0]);
        c->stats.max_eye_depth = static_cast<int64_t>(mx[1]);
        c->stats.max_queries = static_cast<int64_t>(mx[2]);
        unsigned long long sq[4];
        HIP_TRY(hipMemcpy(sq, c->counters + BDPT_NUM_COUNTERS + 3, sizeof(sq), hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; i++) c->stats.sched[i] = static_cast<int64_t>(sq[i]);
        if (c->diag_pending) {
            unsigned long long d[dev::kDiagWords];
            HIP_TRY(hipMemcpy(d, c->diag, sizeof(d), hipMemcpyDeviceToHost));
            const double tick_ms = 1.0 / c->wall_khz;
            if (d[dev::kDiagStart] != ~0ull && d[dev::kDiagEnd] >= d[dev::kDiagStart])
                c->stats.span_ms = static_cast<double>(d[dev::kDiagEnd] - d[dev::kDiagStart]) * tick_ms;
            if (d[dev::kDiagLastClaim] && d[dev::kDiagEnd] >= d[dev::kDiagLastClaim])
                c->stats.tail_ms = static_cast<double>(d[dev::kDiagEnd] - d[dev::kDiagLastClaim]) * tick_ms;
            c->stats.schedule_errors = static_cast<int64_t>(d[dev::kDiagErrors]);
            c->stats.parked_samples = static_cast<int64_t>(d[dev::kDiagParked]);
            c->stats.rr_long_walks_max = static_cast<int64_t>(d[dev::kDiagLongMax]);
            for (int k = 0; k < 3; k++) c->stats.rr_express_iters[k] = static_cast<int64_t>(d[dev::kDiagExpress1 + k]);
        }
        c->pending_timing = false;
    }
    *out = c->stats;
    return BDPT_OK;
}

// out[0]: the frame kernels' grid in blocks, out[1]: the lane slots (read-only; nothing is launched)
int bdpt_get_grid(const bdpt_ctx* c, int64_t out[2]) {
    if (!c || !out) return fail(BDPT_ERR_INVALID, "null argument");
    out[0] = c->grid;
    out[1] = c->nslots;
    return BDPT_OK;
}

// out[0]: checked re-walks, out[1]: closest hits applied, of the last BDPT frame render, a counting
// pass of a build with the deferred reference-leaf check (dev::kDiagLeafRewalks, kDiagLeafHits); 0
// for every other render.
int bdpt_get_leaf_rewalks(bdpt_ctx* c, int64_t out[2]) {
    if (!c || !out) return fail(BDPT_ERR_INVALID, "null argument");
    out[0] = out[1] = 0;
    if (!c->diag_pending) return BDPT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    static_assert(dev::kDiagLeafHits == dev::kDiagLeafRewalks + 1, "two consecutive words");
    unsigned long long w[2] = {0, 0};
    HIP_TRY(hipMemcpy(w, c->diag + dev::kDiagLeafRewalks, sizeof(w), hipMemcpyDeviceToHost));
    out[0] = static_cast<int64_t>(w[0]), out[1] = static_cast<int64_t>(w[1]);
    return BDPT_OK;
}

int bdpt_synchronize(bdpt_ctx* c) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    return BDPT_OK;
}

static int render_bdpt_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, float* fb_host,
                            const Planes& pl = Planes{}) {
    if (!c || !fb_host) return fail(BDPT_ERR_INVALID, "null argument");
    int rc = check_params(p);
    if (rc) return rc;
    if ((rc = check_window(p, w))) return rc;
    if (pl.kind && (rc = check_planes(c, p, pl))) return rc;  // before the planes are staged
    if ((rc = check_pixel_list(c, p, pl))) return rc;
    if ((rc = stage_host(c, fb_host, static_cast<size_t>(p->width) * p->height * 3 * pl.planes(),
                         [&](float* fb) { return render_bdpt(c, p, w, fb, c->stream, pl); })))
        return rc;
    {
        bdpt_stats st;
        if ((rc = bdpt_get_stats(c, &st))) return rc;
        if (st.schedule_errors)
            return fail(BDPT_ERR_HIP, std::to_string(st.schedule_errors) +
                                          " schedule errors (MT19937 draws past the generated ring, or a continuation walk "
                                          "out of stack)");
        if (p->russian_roulette && st.capped_samples)
            return fail(BDPT_ERR_UNSUPPORTED, std::to_string(st.capped_samples) +
                                                  " samples met the Russian-roulette bounds (light-vertex store / "
                                                  "bounce guard); the image is not the reference's");
    }
    return BDPT_OK;
}

int bdpt_render_host(bdpt_ctx* c, const bdpt_frame_params* p, float* fb_host) {
    return render_bdpt_host(c, p, nullptr, fb_host);
}

int bdpt_render_layers_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, int32_t n_layers,
                            float* fb_layers_host) {
    return render_bdpt_host(c, p, w, fb_layers_host, Planes{&kLayerPlanes, n_layers});
}

int bdpt_strategies_sheet_host(bdpt_ctx* c, const float* planes, int32_t n_s, int32_t n_t, int32_t width, int32_t height,
                               const float* gains, float* out) {
    if (!c || !planes || !out) return fail(BDPT_ERR_INVALID, "null argument");
    // a shape the device form refuses: refused by it (its first checks, which read no pointer) before anything is staged
    const bool shape_ok = strategy_shape_ok(n_s, n_t) && width > 0 && height > 0 &&
                          static_cast<int64_t>(n_s) * n_t * width * height * 3 < (int64_t{1} << 31);
    if (!shape_ok) return bdpt_strategies_sheet(c, planes, n_s, n_t, width, height, gains, out, c->stream);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = static_cast<size_t>(n_s) * n_t * width * height * 3;
    HIP_TRY(c->tmp_fb.reserve(2 * n * sizeof(float)));
    float *din = c->tmp_fb, *dout = c->tmp_fb + n;
    HIP_TRY(hipMemcpyAsync(din, planes, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = bdpt_strategies_sheet(c, din, n_s, n_t, width, height, gains, dout, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// both arrays staged in tmp_fb, as bdpt_strategies_sheet_host stages its two
int bdpt_group_planes_combine_host(bdpt_ctx* c, const float* planes, int32_t n_groups, int32_t n_inner, int32_t width,
                                   int32_t height, const float* gains, const float* weights, float* out) {
    if (!c || !planes || !out) return fail(BDPT_ERR_INVALID, "null argument");
    // a shape the device form refuses: refused by it (its first checks, which read no pointer) before anything is staged
    if (check_combine_shape(kCrossedPlanes.entry, kCrossedPlanes, n_groups, width, height, n_inner))
        return bdpt_group_planes_combine(c, planes, n_groups, n_inner, width, height, gains, weights, out, c->stream);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = static_cast<size_t>(width) * height * 3, nin = n * n_groups * n_inner;
    HIP_TRY(c->tmp_fb.reserve((nin + n) * sizeof(float)));
    float *din = c->tmp_fb, *dout = c->tmp_fb + nin;
    HIP_TRY(hipMemcpyAsync(din, planes, nin * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = bdpt_group_planes_combine(c, din, n_groups, n_inner, width, height, gains, weights, dout, c->stream))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_render_group_layers_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                                  const int32_t* group_of_emitter, int32_t n_groups, int32_t n_layers,
                                  float* fb_planes_host) {
    return render_bdpt_host(c, p, w, fb_planes_host, group_layer_planes(group_of_emitter, n_groups, n_layers));
}

int bdpt_render_group_strategies_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                                      const int32_t* group_of_emitter, int32_t n_groups, int32_t n_s, int32_t n_t,
                                      int32_t weighting, float* fb_planes_host) {
    return render_bdpt_host(c, p, w, fb_planes_host,
                            group_strategy_planes(group_of_emitter, n_groups, n_s, n_t, weighting));
}

int bdpt_render_strategies_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, int32_t n_s,
                                int32_t n_t, int32_t weighting, float* fb_planes_host) {
    return render_bdpt_host(c, p, w, fb_planes_host, strategy_planes(n_s, n_t, weighting));
}

int bdpt_render_light_groups_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                                  int32_t n_groups, const int32_t* group_of_emitter, float* fb_groups_host) {
    return render_bdpt_host(c, p, w, fb_groups_host, Planes{&kGroupPlanes, n_groups, group_of_emitter});
}

// Sample windows: the three integrators' frame entries with a window (null: the whole
// range, then exactly the unwindowed entry).
static int window_integrator(const bdpt_path_params* path, const bdpt_direct_params* direct) {
    if (path && direct) return fail(BDPT_ERR_INVALID, "bdpt_render_window: path and direct are both set (at most one)");
    return BDPT_OK;
}
int bdpt_render_window(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                       const bdpt_path_params* path, const bdpt_direct_params* direct, float* fb, void* hip_stream) {
    if (int rc = window_integrator(path, direct)) return rc;
    if (path) return render_path(c, p, w, path, fb, hip_stream);
    if (direct) return render_direct(c, p, w, direct, fb, hip_stream);
    return render_bdpt(c, p, w, fb, hip_stream);
}
int bdpt_render_window_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w,
                            const bdpt_path_params* path, const bdpt_direct_params* direct, float* fb_host) {
    if (int rc = window_integrator(path, direct)) return rc;
    if (path) return render_path_host(c, p, w, path, fb_host);
    if (direct) return render_direct_host(c, p, w, direct, fb_host);
    return render_bdpt_host(c, p, w, fb_host);
}

static int render_bdpt_sample(bdpt_ctx* c, const bdpt_frame_params* p, const float ray[8], uint32_t* state,
                              float Li[3], bdpt_splat* splats, int32_t capacity, int32_t* nsplats, uint32_t* taken) {
    if (!c || !ray || !Li || !nsplats || (capacity > 0 && !splats) || capacity < 0)
        return fail(BDPT_ERR_INVALID, "null argument");
    int rc = check_params(p);
    if (rc) return rc;
    if ((rc = check_mt_state(state))) return rc;
    if ((rc = textured_frame_check(c, p))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the sample kernel's one lane uses lane slot 0 of the light-vertex store
    if ((rc = ensure_lv(c, make_frame(p).lv_max, 1))) return rc;
    // a sample splats at most once per light vertex: rr_depth bounds the list
    // without Russian roulette; with it the list grows on demand (below)
    if ((rc = ensure_sample_buffers(c, std::max(p->rr_depth, 1)))) return rc;
    dev::DevFrame fr = make_frame(p);
    fr.capped = c->capped;
    dev::DevScene sc = c->sc;
    sc.mt_ring = c->mt_state;  // the sample kernel's generator state (mt_state_u32)
    const float* origins[2] = {p->camera.eye, ray};  // camera connections start at the eye, the walk at ray.o
    sc.node_slack = node_slack_needed(c, origins, 2);
    const dev::Ray r{dev::f3{ray[0], ray[1], ray[2]}, dev::f3{ray[3], ray[4], ray[5]}, ray[6], ray[7]};
    uint32_t st_out[BDPT_MT19937_WORDS];
    std::vector<float> list;
    float out[4];
    uint32_t n = 0;
    for (int attempt = 0;; attempt++) {
        if ((rc = begin_use(c, c->stream))) return rc;
        const uint32_t hdr[4] = {0u, static_cast<uint32_t>(c->splat_cap), 0u, 0u};
        HIP_TRY(hipMemcpyAsync(c->mt_state, state, sizeof(uint32_t) * BDPT_MT19937_WORDS, hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMemcpyAsync(c->splat_list, hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->capped, 0, sizeof(uint32_t), c->stream));
        HIP_TRY((c->textured ? launch_sample_tex : launch_sample)(sc, fr, c->splat_list, c->lv, c->gstack, r,
                                                                  c->sample_out, c->stream));
        list.assign(4 * (static_cast<size_t>(c->splat_cap) + 1), 0.f);
        HIP_TRY(hipMemcpyAsync(out, c->sample_out, sizeof(out), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(list.data(), c->splat_list, list.size() * sizeof(float), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipMemcpyAsync(st_out, c->mt_state, sizeof(st_out), hipMemcpyDeviceToHost, c->stream));
        uint32_t capped = 0;
        HIP_TRY(hipMemcpyAsync(&capped, c->capped, sizeof(capped), hipMemcpyDeviceToHost, c->stream));
        if ((rc = end_use(c, c->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (capped)
            return fail(BDPT_ERR_UNSUPPORTED, "the sample met the Russian-roulette bounds (light-vertex store / "
                                              "bounce guard)");
        std::memcpy(&n, &list[0], 4);
        if (n <= static_cast<uint32_t>(c->splat_cap)) break;
        // more splats than the device list holds (the kernel counts them all):
        // grow it and run the sample again from the caller's unchanged state
        if (attempt > 0) return fail(BDPT_ERR_HIP, "splat list overflow");
        if ((rc = ensure_sample_buffers(c, static_cast<int32_t>(n)))) return rc;
    }
    *nsplats = static_cast<int32_t>(n);
    if (static_cast<int32_t>(n) > capacity)  // the caller's state is left as it was
        return fail(BDPT_ERR_INVALID, "splat capacity too small (" + std::to_string(n) + " splats)");
    for (uint32_t k = 0; k < n; k++) {
        const float* e = &list[4 + 4 * static_cast<size_t>(k)];
        std::memcpy(&splats[k].pixel, &e[0], 4);
        splats[k].rgb[0] = e[1], splats[k].rgb[1] = e[2], splats[k].rgb[2] = e[3];
    }
    std::memcpy(state, st_out, sizeof(st_out));
    Li[0] = out[0], Li[1] = out[1], Li[2] = out[2];
    if (taken) std::memcpy(taken, &out[3], 4);
    return BDPT_OK;
}

int bdpt_sampler_state(uint32_t seed, int64_t draws, uint32_t state[BDPT_MT19937_WORDS]) {
    if (!state || draws < 0) return fail(BDPT_ERR_INVALID, "bad argument");
    mt19937_state(seed, draws, state);
    return BDPT_OK;
}

int bdpt_render_sample_mt(bdpt_ctx* c, const bdpt_frame_params* p, const float ray[8],
                          uint32_t state[BDPT_MT19937_WORDS], float Li[3], bdpt_splat* splats, int32_t capacity,
                          int32_t* nsplats) {
    return render_bdpt_sample(c, p, ray, state, Li, splats, capacity, nsplats, nullptr);
}

int bdpt_render_sample(bdpt_ctx* c, const bdpt_frame_params* p, const float ray[8], uint32_t seed,
                       int32_t* draws, float Li[3], float* fb_host) {
    if (!c || !p || !draws || !fb_host) return fail(BDPT_ERR_INVALID, "null argument");
    if (*draws < 0) return fail(BDPT_ERR_INVALID, "negative draw count");
    uint32_t st[BDPT_MT19937_WORDS], used = 0;
    mt19937_state(seed, *draws, st);
    std::vector<bdpt_splat> sp(static_cast<size_t>(std::max(p->rr_depth, 1)));
    int32_t n = 0;
    int rc = render_bdpt_sample(c, p, ray, st, Li, sp.data(), static_cast<int32_t>(sp.size()), &n, &used);
    if (rc == BDPT_ERR_INVALID && n > static_cast<int32_t>(sp.size())) {  // Russian roulette: a longer list
        sp.resize(static_cast<size_t>(n));
        rc = render_bdpt_sample(c, p, ray, st, Li, sp.data(), n, &n, &used);
    }
    if (rc) return rc;
    for (int32_t k = 0; k < n; k++) {  // rgb[pixel] += radiance * misWeight, in the sample's order
        float* px = fb_host + 3 * static_cast<size_t>(sp[k].pixel);
        px[0] += sp[k].rgb[0], px[1] += sp[k].rgb[1], px[2] += sp[k].rgb[2];
    }
    *draws += static_cast<int32_t>(used);
    return BDPT_OK;
}

// build: BDPT_KAT_EXACT / _FAST / _NG, the compilation of the BSDF kernel to run
static int bsdf_kat(bdpt_ctx* c, int mode, int64_t n, const int32_t* mat, const float* wo, const float* x,
                    float* out, int out_per, int build = BDPT_KAT_EXACT) {
    if (!c || n < 0 || (n > 0 && (!mat || !wo || !x || !out))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (build < BDPT_KAT_EXACT || build > BDPT_KAT_NG) return fail(BDPT_ERR_INVALID, "bad build");
    if (build == BDPT_KAT_NG && !ng_table(c))
        return fail(BDPT_ERR_UNSUPPORTED, "the build without glossy lobes serves material tables of diffuse, mirror "
                                          "and glass records only; this scene has a Mixture / Phong or null BSDF");
    for (int64_t i = 0; i < n; i++)
        if (mat[i] < 0 || mat[i] >= c->sc.nbsdf) return fail(BDPT_ERR_INVALID, "material index out of range");
    for (int64_t i = 0; c->textured && i < n; i++)
        if (c->mat_textured[mat[i]])
            return fail(BDPT_ERR_UNSUPPORTED, "bdpt_bsdf_eval / pdf / sample / eval_pdfs / local_for of material " +
                                                  std::to_string(mat[i]) +
                                                  ": it reads a bitmap texture and these calls carry no hit (texture + "
                                                  "bdpt_bsdf_*)");
    if (n == 0) return BDPT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = begin_use(c, c->stream))) return rc;
    DevBuf<int32_t> dm;
    DevBuf<float> dwo, dx, dout;
    const size_t N = static_cast<size_t>(n);
    if ((rc = kat_in(c, dm, mat, 4 * N)) || (rc = kat_in(c, dwo, wo, 12 * N)) ||
        (rc = kat_in(c, dx, x, (mode == 2 ? 8 : 12) * N)) || (rc = kat_in<float>(c, dout, nullptr, 4 * out_per * N)))
        return rc;
    const auto launch = build == BDPT_KAT_FAST ? launch_bsdf_kat_fw : build == BDPT_KAT_NG ? launch_bsdf_kat_ng
                                                                                            : launch_bsdf_kat;
    HIP_TRY(launch(c->sc, mode, n, dm, dwo, dx, dout, c->stream));
    HIP_TRY(hipMemcpyAsync(out, dout, 4 * out_per * N, hipMemcpyDeviceToHost, c->stream));
    if ((rc = end_use(c, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_bsdf_eval(bdpt_ctx* c, int64_t n, const int32_t* mat, const float* wo, const float* wi, float* f) {
    return bsdf_kat(c, 0, n, mat, wo, wi, f, 3);
}

int bdpt_bsdf_pdf(bdpt_ctx* c, int64_t n, const int32_t* mat, const float* wo, const float* wi, float* pdf) {
    return bsdf_kat(c, 1, n, mat, wo, wi, pdf, 1);
}

int bdpt_bsdf_sample(bdpt_ctx* c, int64_t n, const int32_t* mat, const float* wo, const float* u, float* f,
                     float* wi, float* pdf) {
    if (n > 0 && (!f || !wi || !pdf)) return fail(BDPT_ERR_INVALID, "null output");
    std::vector<float> o(7 * static_cast<size_t>(std::max<int64_t>(n, 0)));
    int rc = bsdf_kat(c, 2, n, mat, wo, u, o.data(), 7);
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++) {
        const float* r = &o[7 * static_cast<size_t>(i)];
        f[3 * i] = r[0], f[3 * i + 1] = r[1], f[3 * i + 2] = r[2];
        wi[3 * i] = r[3], wi[3 * i + 1] = r[4], wi[3 * i + 2] = r[5];
        pdf[i] = r[6];
    }
    return BDPT_OK;
}

int bdpt_bsdf_eval_pdfs(bdpt_ctx* c, int32_t build, int64_t n, const int32_t* mat, const float* wo, const float* wi,
                        float* out) {
    return bsdf_kat(c, 3, n, mat, wo, wi, out, 5, build);
}

int bdpt_bsdf_local_for(bdpt_ctx* c, int32_t build, int64_t n, const int32_t* mat, const float* nrm, const float* v,
                        float* out) {
    return bsdf_kat(c, 4, n, mat, nrm, v, out, 3, build);
}

int bdpt_bsdf_type(const bdpt_scene* s, int32_t mat, uint32_t* type, int32_t* kind) {
    if (!s || !type || !kind) return fail(BDPT_ERR_INVALID, "null argument");
    if (mat < 0 || mat >= static_cast<int32_t>(s->layout.bsdfs.size()))
        return fail(BDPT_ERR_INVALID, "material index out of range");
    *type = s->layout.bsdfs[static_cast<size_t>(mat)].type;
    *kind = s->layout.bsdfs[static_cast<size_t>(mat)].kind;
    return BDPT_OK;
}

int bdpt_intersect(bdpt_ctx* c, int64_t n, const float* rays, int32_t occlusion, bdpt_hit* out) {
    return bdpt_intersect_from(c, n, rays, nullptr, nullptr, occlusion, out);
}

int bdpt_intersect_from(bdpt_ctx* c, int64_t n, const float* rays, const float* origin_normals,
                        const int32_t* origin_tris, int32_t occlusion, bdpt_hit* out) {
    static_assert(sizeof(bdpt_hit) == 20 * 4, "bdpt_hit is the kernel's 20-word record");
    if (!c || n < 0 || (n > 0 && (!rays || !out))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (n == 0) return BDPT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = begin_use(c, c->stream))) return rc;
    DevBuf<float> dr, dout, dn;
    DevBuf<int32_t> dt;
    const size_t N = static_cast<size_t>(n);
    if (origin_tris)
        for (size_t i = 0; i < N; i++)
            if (origin_tris[i] < -1 || origin_tris[i] >= c->ntri) return fail(BDPT_ERR_INVALID, "origin_tris out of range");
    if ((rc = kat_in(c, dr, rays, 32 * N)) || (rc = kat_in<float>(c, dout, nullptr, 80 * N))) return rc;
    if (origin_normals && (rc = kat_in(c, dn, origin_normals, 12 * N))) return rc;
    if (origin_normals && origin_tris && (rc = kat_in(c, dt, origin_tris, 4 * N))) return rc;
    // The interior-box test the frame kernels would use for these origins: without
    // the ambiguity slack when every origin lies within 100 scene diagonals (as
    // for a frame whose camera does, node_slack_needed), with it otherwise.
    std::vector<const float*> origins(N);
    for (size_t i = 0; i < N; i++) origins[i] = rays + 8 * i;
    dev::DevScene sc = c->sc;
    sc.node_slack = node_slack_needed(c, origins.data(), static_cast<int>(std::min<size_t>(N, 0x7fffffff)));
    // the traversal-stack overflow columns serve c->nslots rays at a time
    for (int64_t b = 0; b < n; b += c->nslots) {
        const int64_t m = std::min<int64_t>(c->nslots, n - b);
        HIP_TRY(launch_intersect_kat(sc, m, occlusion ? 1 : 0, dr + 8 * b, dn ? dn + 3 * b : nullptr,
                                     dt ? dt + b : nullptr, c->gstack, c->nslots, dout + 20 * b, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(out, dout, 80 * N, hipMemcpyDeviceToHost, c->stream));
    if ((rc = end_use(c, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// The closest hits of bdpt_intersect_from through the deferred reference-leaf check of the
// frame kernels (kat_leaf_defer.hip); rewalked (optional): per ray, 1 when its winner failed the
// check and the query was walked again. BDPT_LEAF_RECHECK=1 (a debugging knob) fails every check.
int bdpt_intersect_deferred(bdpt_ctx* c, int64_t n, const float* rays, const float* origin_normals,
                            const int32_t* origin_tris, bdpt_hit* out, int32_t* rewalked) {
    if (!c || n < 0 || (n > 0 && (!rays || !out))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (n == 0) return BDPT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = begin_use(c, c->stream))) return rc;
    DevBuf<float> dr, dout, dn;
    DevBuf<int32_t> dt, dre;
    const size_t N = static_cast<size_t>(n);
    if (origin_tris)
        for (size_t i = 0; i < N; i++)
            if (origin_tris[i] < -1 || origin_tris[i] >= c->ntri) return fail(BDPT_ERR_INVALID, "origin_tris out of range");
    if ((rc = kat_in(c, dr, rays, 32 * N)) || (rc = kat_in<float>(c, dout, nullptr, 80 * N)) ||
        (rc = kat_in<int32_t>(c, dre, nullptr, 4 * N)))
        return rc;
    if (origin_normals && (rc = kat_in(c, dn, origin_normals, 12 * N))) return rc;
    if (origin_normals && origin_tris && (rc = kat_in(c, dt, origin_tris, 4 * N))) return rc;
    std::vector<const float*> origins(N);
    for (size_t i = 0; i < N; i++) origins[i] = rays + 8 * i;
    dev::DevScene sc = c->sc;
    sc.node_slack = node_slack_needed(c, origins.data(), static_cast<int>(std::min<size_t>(N, 0x7fffffff)));
    const int force = leaf_recheck_knob() ? 1 : 0;
    for (int64_t b = 0; b < n; b += c->nslots) {  // (the traversal-stack overflow columns serve c->nslots rays)
        const int64_t m = std::min<int64_t>(c->nslots, n - b);
        HIP_TRY(launch_intersect_defer(sc, m, c->textured ? 1 : 0, force, dr + 8 * b, dn ? dn + 3 * b : nullptr,
                                       dt ? dt + b : nullptr, c->gstack, c->nslots, dout + 20 * b, dre + b, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(out, dout, 80 * N, hipMemcpyDeviceToHost, c->stream));
    if (rewalked) HIP_TRY(hipMemcpyAsync(rewalked, dre, 4 * N, hipMemcpyDeviceToHost, c->stream));
    if ((rc = end_use(c, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// ---- first-hit feature buffers and the filter for preview frames (aov_kernels.hip) ----
static int check_aov_params(const bdpt_frame_params* p) {
    if (int rc = check_frame_size(p)) return rc;
    if (p->flags != 0) return fail(BDPT_ERR_UNSUPPORTED, "bdpt_render_aov: flags must be 0 (no counting pass or full traversal)");
    return check_row_shard(p);
}

int bdpt_render_aov(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, float* aov,
                    void* hip_stream) {
    if (!c || !aov) return fail(BDPT_ERR_INVALID, "null argument");
    int rc = check_aov_params(p);
    if (rc) return rc;
    if ((rc = check_window(p, w))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const dev::DevFrame fr = make_frame(p, w);
    dev::DevScene sc = c->sc;
    const float* eye[1] = {p->camera.eye};
    sc.node_slack = node_slack_needed(c, eye, 1);  // the interior-box test a frame of this camera uses
    if (!sc.tex_tab) sc.tex_tab = static_cast<const float4*>(c->aov_no_tex);
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    HIP_TRY(launch_aov(sc, fr, c->aov_mats, aov, c->gstack, c->nslots, st));
    return end_timed(c, st, static_cast<int64_t>(fr.total_samples), fr.total_samples > 0 ? 1 : 0);
}

int bdpt_render_aov_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, float* aov_host) {
    if (!c || !aov_host) return fail(BDPT_ERR_INVALID, "null argument");
    int rc = check_aov_params(p);
    if (rc) return rc;
    if ((rc = check_window(p, w))) return rc;
    return stage_host(c, aov_host, static_cast<size_t>(p->width) * p->height * 8,
                      [&](float* aov) { return bdpt_render_aov(c, p, w, aov, c->stream); });
}

// The frame size and the parameter fields, for bdpt_denoise and bdpt_denoise_planes (entry: whose message).
static int check_denoise_fields(const std::string& entry, int32_t width, int32_t height, const bdpt_denoise_params* d) {
    if (width <= 0 || height <= 0 || static_cast<int64_t>(width) * height >= (1ll << 31))
        return fail(BDPT_ERR_INVALID, entry + ": width/height must be > 0 and W*H fit int32");
    if (d->iterations < 0 || d->iterations > 8) return fail(BDPT_ERR_INVALID, entry + ": iterations must be in [0, 8]");
    if (!(d->sigma_color > 0.f)) return fail(BDPT_ERR_INVALID, entry + ": sigma_color must be > 0");
    if (!(d->sigma_normal > 0.f)) return fail(BDPT_ERR_INVALID, entry + ": sigma_normal must be > 0");
    if (!(d->sigma_depth > 0.f)) return fail(BDPT_ERR_INVALID, entry + ": sigma_depth must be > 0");
    if (d->demodulate != 0 && d->demodulate != 1) return fail(BDPT_ERR_INVALID, entry + ": demodulate must be 0 or 1");
    if (!(d->norm > 0.f) || !std::isfinite(d->norm)) return fail(BDPT_ERR_INVALID, entry + ": norm must be > 0");
    return BDPT_OK;
}

static int check_denoise(int32_t width, int32_t height, const float* color, const float* aov, const float* out,
                         const bdpt_denoise_params* d) {
    if (!color || !aov || !out || !d) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_denoise_fields("bdpt_denoise", width, height, d)) return rc;
    const size_t px = static_cast<size_t>(width) * height;
    auto overlaps = [&](const float* a, size_t na) {
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + px * 3 * sizeof(float);
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + na * sizeof(float);
        return o0 < a1 && a0 < o1;
    };
    if (overlaps(color, px * 3)) return fail(BDPT_ERR_INVALID, "bdpt_denoise: out overlaps color");
    if (overlaps(aov, px * 8)) return fail(BDPT_ERR_INVALID, "bdpt_denoise: out overlaps aov");
    return BDPT_OK;
}

// The filter scratch of bdpt_denoise and bdpt_denoise_var (packed guides and the two images, 64 bytes per
// pixel), grown when a larger frame comes.
static int reserve_denoise_scratch(bdpt_ctx* c, size_t px) {
    if (px <= c->dn_pixels) return BDPT_OK;
    c->dn_pixels = 0;
    HIP_TRY(c->dn_guide.reserve(px * 32));
    HIP_TRY(c->dn_img[0].reserve(px * 16));
    HIP_TRY(c->dn_img[1].reserve(px * 16));
    c->dn_pixels = px;
    return BDPT_OK;
}

int bdpt_denoise(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const float* aov, float* out,
                 const bdpt_denoise_params* d, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_denoise(width, height, color, aov, out, d);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t px = static_cast<size_t>(width) * height;
    if ((rc = begin_use(c, st))) return rc;
    if (d->iterations > 0 && (rc = reserve_denoise_scratch(c, px))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    if (d->iterations == 0) {
        HIP_TRY(launch_denoise_scale(px * 3, color, d->norm, out, st));
    } else {
        HIP_TRY(launch_denoise_prepare(width, height, color, aov, d->norm, d->demodulate, c->dn_guide, c->dn_img[0], st));
        const float inv_n = 1.f / (d->sigma_normal * d->sigma_normal);
        for (int i = 0; i < d->iterations; i++) {
            const float sc_i = d->sigma_color * std::ldexp(1.f, -i);
            HIP_TRY(launch_denoise_iter(width, height, 1 << i, 1.f / (sc_i * sc_i), inv_n, d->sigma_depth, d->demodulate,
                                        c->dn_guide, c->dn_img[i & 1], c->dn_img[(i + 1) & 1], out,
                                        i + 1 == d->iterations, st));
        }
    }
    return end_timed(c, st, 0, d->iterations == 0 ? 1 : d->iterations + 1);
}

int bdpt_denoise_host(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const float* aov, float* out,
                      const bdpt_denoise_params* d) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_denoise(width, height, color, aov, out, d);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = static_cast<size_t>(width) * height;
    HIP_TRY(c->tmp_fb.reserve(px * 14 * sizeof(float)));
    float *dc = c->tmp_fb, *da = c->tmp_fb + px * 3, *dout = c->tmp_fb + px * 11;  // color, aov (16-byte aligned or not: scalar loads), out
    HIP_TRY(hipMemcpyAsync(dc, color, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(da, aov, px * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_denoise(c, width, height, dc, da, dout, d, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// ---- per-pixel moments across sample batches, and the filter guided by them (aov_kernels.hip) ----
struct FloatSpan {
    const char* name;
    const float* p;
    size_t floats;
};
static bool spans_overlap(const FloatSpan& a, const FloatSpan& b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a.p && b.p && a0 < b0 + b.floats * sizeof(float) && b0 < a0 + a.floats * sizeof(float);
}

static int check_batch_moments(int32_t width, int32_t height, int32_t n_batches, const float* planes, const float* out_sum,
                               const float* out_var) {
    const std::string entry = "bdpt_batch_moments";
    if (width <= 0 || height <= 0) return fail(BDPT_ERR_INVALID, entry + ": width/height must be > 0");
    if (n_batches < 2 || n_batches > 64) return fail(BDPT_ERR_INVALID, entry + ": n_batches must be in [2, 64]");
    const uint64_t px = static_cast<uint64_t>(width) * static_cast<uint64_t>(height);
    if (px >= (1ull << 30) || static_cast<uint64_t>(n_batches) * px >= (1ull << 30))
        return fail(BDPT_ERR_INVALID, entry + ": n_batches * width * height must be below 2^30");
    if (!planes) return fail(BDPT_ERR_INVALID, entry + ": planes must not be NULL");
    if (!out_var) return fail(BDPT_ERR_INVALID, entry + ": out_var must not be NULL");
    const FloatSpan in = {"planes", planes, n_batches * px * 3};
    const FloatSpan sum = {"out_sum", out_sum, px * 3}, var = {"out_var", out_var, px * 3};
    if (spans_overlap(sum, in)) return fail(BDPT_ERR_INVALID, entry + ": out_sum overlaps planes");
    if (spans_overlap(var, in)) return fail(BDPT_ERR_INVALID, entry + ": out_var overlaps planes");
    if (spans_overlap(var, sum)) return fail(BDPT_ERR_INVALID, entry + ": out_var overlaps out_sum");
    return BDPT_OK;
}

int bdpt_batch_moments(bdpt_ctx* c, int32_t width, int32_t height, int32_t n_batches, const float* planes, float* out_sum,
                       float* out_var, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_batch_moments(width, height, n_batches, planes, out_sum, out_var);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    const float scale = static_cast<float>(n_batches) / static_cast<float>(n_batches - 1);
    HIP_TRY(launch_batch_moments(planes, static_cast<size_t>(width) * height * 3, n_batches, scale, out_sum, out_var, st));
    return end_timed(c, st, 0, 1);
}

int bdpt_batch_moments_host(bdpt_ctx* c, int32_t width, int32_t height, int32_t n_batches, const float* planes,
                            float* out_sum, float* out_var) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_batch_moments(width, height, n_batches, planes, out_sum, out_var);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = static_cast<size_t>(width) * height * 3, all = n * n_batches;
    HIP_TRY(c->tmp_fb.reserve((all + 2 * n) * sizeof(float)));
    float *dp = c->tmp_fb, *dsum = dp + all, *dvar = dsum + n;  // planes, out_sum, out_var
    HIP_TRY(hipMemcpyAsync(dp, planes, all * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_batch_moments(c, width, height, n_batches, dp, out_sum ? dsum : nullptr, dvar, c->stream))) return rc;
    if (out_sum) HIP_TRY(hipMemcpyAsync(out_sum, dsum, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_var, dvar, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// ---------------------------------------------------------------- adaptive sampling
int bdpt_render_pixels(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, const int32_t* pixels,
                       int32_t n_pixels, float* fb, void* hip_stream) {
    if (n_pixels < 0) return fail(BDPT_ERR_INVALID, "bdpt_render_pixels: n_pixels must be in [0, width * height]");
    return render_bdpt(c, p, w, fb, hip_stream, pixel_planes(pixels, n_pixels));
}

int bdpt_render_pixels_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_sample_window* w, const int32_t* pixels,
                            int32_t n_pixels, float* fb_host) {
    const std::string entry = "bdpt_render_pixels: ";
    if (!c || !fb_host) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(p)) return rc;
    const int64_t npx = static_cast<int64_t>(p->width) * p->height;
    if (n_pixels < 0 || n_pixels > npx) return fail(BDPT_ERR_INVALID, entry + "n_pixels must be in [0, width * height]");
    if (n_pixels > 0 && !pixels) return fail(BDPT_ERR_INVALID, entry + "pixels must not be NULL");
    // the list's contract, which the device form trusts: inside the image, strictly ascending
    for (int32_t i = 0; i < n_pixels; i++) {
        if (pixels[i] < 0 || pixels[i] >= npx)
            return fail(BDPT_ERR_INVALID, entry + "pixels[" + std::to_string(i) + "] = " + std::to_string(pixels[i]) +
                                              " is outside [0, width * height)");
        if (i > 0 && pixels[i] <= pixels[i - 1])
            return fail(BDPT_ERR_INVALID, entry + "pixels[" + std::to_string(i) + "] = " + std::to_string(pixels[i]) +
                                              " does not ascend (the list must be strictly ascending)");
    }
    // every refusal before the list is uploaded (render_bdpt_host repeats them before it stages the planes)
    Planes pl = pixel_planes(n_pixels > 0 ? pixels : nullptr, n_pixels);
    int rc = check_params(p);
    if (rc || (rc = check_window(p, w)) || (rc = check_planes(c, p, pl)) || (rc = check_pixel_list(c, p, pl))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->pixel_list.reserve(std::max<size_t>(sizeof(int32_t) * static_cast<size_t>(n_pixels), 16)));
    if (n_pixels > 0)
        HIP_TRY(hipMemcpy(c->pixel_list, pixels, sizeof(int32_t) * static_cast<size_t>(n_pixels), hipMemcpyHostToDevice));
    pl.pixels = c->pixel_list;
    return render_bdpt_host(c, p, w, fb_host, pl);
}

static bool finite_nonneg(float x) { return std::isfinite(x) && x >= 0.f; }

static int check_adaptive_resolve(int32_t width, int32_t height, int32_t n_batches, int32_t spp, const void* planes,
                                  const void* m, const void* out_sum, const void* out_var) {
    const std::string entry = "bdpt_adaptive_resolve: ";
    if (width <= 0 || height <= 0) return fail(BDPT_ERR_INVALID, entry + "width/height must be > 0");
    if (n_batches < 2 || n_batches > 64) return fail(BDPT_ERR_INVALID, entry + "n_batches must be in [2, 64]");
    if (spp < 1) return fail(BDPT_ERR_INVALID, entry + "spp must be >= 1");
    if (2ull * static_cast<uint64_t>(n_batches) * static_cast<uint64_t>(width) * static_cast<uint64_t>(height) >= (1ull << 30))
        return fail(BDPT_ERR_INVALID, entry + "2 * n_batches * width * height must be below 2^30");
    if (!planes) return fail(BDPT_ERR_INVALID, entry + "planes must not be NULL");
    if (!m) return fail(BDPT_ERR_INVALID, entry + "samples_per_batch must not be NULL");
    if (!out_sum) return fail(BDPT_ERR_INVALID, entry + "out_sum must not be NULL");
    if (!out_var) return fail(BDPT_ERR_INVALID, entry + "out_var must not be NULL");
    return BDPT_OK;
}

// t = spp W H / (K M) in double, rounded once (0 when no sample was traced)
static float adaptive_splat_scale(int32_t spp, int32_t width, int32_t height, int32_t K, int64_t M) {
    if (M <= 0) return 0.f;
    return static_cast<float>(static_cast<double>(spp) * width * height / (static_cast<double>(K) * static_cast<double>(M)));
}

// the launch alone, for callers that order and time their own work (the driver)
static int adaptive_resolve_launch(int32_t width, int32_t height, int32_t K, int32_t spp, const float* planes,
                                   const int32_t* m, int64_t M, float* out_sum, float* out_var, hipStream_t st) {
    const float scale = static_cast<float>(K) / static_cast<float>(K - 1);
    HIP_TRY(launch_adaptive_resolve(planes, m, static_cast<size_t>(width) * height * 3, K, spp,
                                    adaptive_splat_scale(spp, width, height, K, M), scale, out_sum, out_var, st));
    return BDPT_OK;
}

int bdpt_adaptive_resolve(bdpt_ctx* c, int32_t width, int32_t height, int32_t n_batches, int32_t spp, const float* planes,
                          const int32_t* m, int64_t splat_total, float* out_sum, float* out_var, void* hip_stream) {
    int rc = check_adaptive_resolve(width, height, n_batches, spp, planes, m, out_sum, out_var);
    if (rc) return rc;
    if (splat_total < 0)
        return fail(BDPT_ERR_INVALID, "bdpt_adaptive_resolve: splat_total must be >= 0 (only the host form counts it)");
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    if ((rc = adaptive_resolve_launch(width, height, n_batches, spp, planes, m, splat_total, out_sum, out_var, st))) return rc;
    return end_timed(c, st, 0, 1);
}

int bdpt_adaptive_resolve_host(bdpt_ctx* c, int32_t width, int32_t height, int32_t n_batches, int32_t spp,
                               const float* planes, const int32_t* m, int64_t splat_total, float* out_sum, float* out_var) {
    int rc = check_adaptive_resolve(width, height, n_batches, spp, planes, m, out_sum, out_var);
    if (rc) return rc;
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    const size_t N = static_cast<size_t>(width) * height, n = N * 3, all = n * 2 * n_batches;
    if (splat_total < 0) {
        splat_total = 0;
        for (size_t i = 0; i < N; i++) splat_total += m[i];
    }
    HIP_TRY(hipSetDevice(c->device));
    // planes, out_sum, out_var (floats, each a multiple of 16 bytes when n is), then m
    const size_t n16 = (n + 3) & ~static_cast<size_t>(3);
    HIP_TRY(c->ad_stage.reserve((all + 2 * n16) * sizeof(float) + N * sizeof(int32_t)));
    float* const dp = static_cast<float*>(c->ad_stage.get());
    float *dsum = dp + all, *dvar = dsum + n16;
    int32_t* const dm = reinterpret_cast<int32_t*>(dvar + n16);
    HIP_TRY(hipMemcpyAsync(dp, planes, all * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dm, m, N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_adaptive_resolve(c, width, height, n_batches, spp, dp, dm, splat_total, dsum, dvar, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out_sum, dsum, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_var, dvar, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

static int check_adaptive_select(int32_t width, int32_t height, const void* sum, const void* var, float threshold, float eps,
                                 int32_t step, int32_t m_max, int32_t dilate, const void* m, const void* list,
                                 const void* count) {
    const std::string entry = "bdpt_adaptive_select: ";
    if (width <= 0 || height <= 0) return fail(BDPT_ERR_INVALID, entry + "width/height must be > 0");
    if (static_cast<uint64_t>(width) * static_cast<uint64_t>(height) >= (1ull << 30))
        return fail(BDPT_ERR_INVALID, entry + "width * height must be below 2^30");
    if (!finite_nonneg(threshold)) return fail(BDPT_ERR_INVALID, entry + "threshold must be finite and >= 0");
    if (!finite_nonneg(eps)) return fail(BDPT_ERR_INVALID, entry + "eps must be finite and >= 0");
    if (step < 1) return fail(BDPT_ERR_INVALID, entry + "step must be >= 1");
    if (m_max < 0) return fail(BDPT_ERR_INVALID, entry + "m_max must be >= 0");
    if (static_cast<int64_t>(m_max) + step >= (int64_t{1} << 31)) return fail(BDPT_ERR_INVALID, entry + "m_max + step must fit int32");
    if (dilate != 0 && dilate != 1) return fail(BDPT_ERR_INVALID, entry + "dilate must be 0 or 1");
    if (!sum || !var) return fail(BDPT_ERR_INVALID, entry + "sum and var must not be NULL");
    if (!m) return fail(BDPT_ERR_INVALID, entry + "samples_per_batch must not be NULL");
    if (!list || !count) return fail(BDPT_ERR_INVALID, entry + "out_list and out_count must not be NULL");
    return BDPT_OK;
}

static int adaptive_select_launch(bdpt_ctx* c, int32_t width, int32_t height, const float* sum, const float* var,
                                  float threshold, float eps, int32_t step, int32_t m_max, int32_t dilate, int32_t* m,
                                  int32_t* list, int32_t* count, hipStream_t st) {
    HIP_TRY(c->ad_scratch.reserve(adaptive_select_scratch_bytes(static_cast<size_t>(width) * height)));
    HIP_TRY(launch_adaptive_select(sum, var, width, height, threshold, eps, step, m_max, dilate, m, list, count, c->ad_scratch, st));
    return BDPT_OK;
}

int bdpt_adaptive_select(bdpt_ctx* c, int32_t width, int32_t height, const float* sum, const float* var, float threshold,
                         float eps, int32_t step, int32_t m_max, int32_t dilate, int32_t* m, int32_t* list, int32_t* count,
                         void* hip_stream) {
    int rc = check_adaptive_select(width, height, sum, var, threshold, eps, step, m_max, dilate, m, list, count);
    if (rc) return rc;
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    if ((rc = adaptive_select_launch(c, width, height, sum, var, threshold, eps, step, m_max, dilate, m, list, count, st)))
        return rc;
    return end_timed(c, st, 0, 3);
}

int bdpt_adaptive_select_host(bdpt_ctx* c, int32_t width, int32_t height, const float* sum, const float* var,
                              float threshold, float eps, int32_t step, int32_t m_max, int32_t dilate, int32_t* m,
                              int32_t* list, int32_t* count) {
    int rc = check_adaptive_select(width, height, sum, var, threshold, eps, step, m_max, dilate, m, list, count);
    if (rc) return rc;
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    const size_t N = static_cast<size_t>(width) * height, n = N * 3;
    HIP_TRY(hipSetDevice(c->device));
    // sum, var (floats), m, list (N int32 each), count
    HIP_TRY(c->ad_stage.reserve(2 * n * sizeof(float) + (2 * N + 4) * sizeof(int32_t)));
    float* const dsum = static_cast<float*>(c->ad_stage.get());
    float* const dvar = dsum + n;
    int32_t* const dm = reinterpret_cast<int32_t*>(dvar + n);
    int32_t *dlist = dm + N, *dcount = dlist + N;
    HIP_TRY(hipMemcpyAsync(dsum, sum, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dvar, var, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dm, m, N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_adaptive_select(c, width, height, dsum, dvar, threshold, eps, step, m_max, dilate, dm, dlist, dcount, c->stream)))
        return rc;
    HIP_TRY(hipMemcpyAsync(count, dcount, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (*count < 0 || static_cast<size_t>(*count) > N) return fail(BDPT_ERR_HIP, "bdpt_adaptive_select: a count outside [0, width * height]");
    HIP_TRY(hipMemcpy(m, dm, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*count > 0) HIP_TRY(hipMemcpy(list, dlist, static_cast<size_t>(*count) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BDPT_OK;
}

// The driver's own parameters (no context needed), then what its pixel-list renders refuse.
static int check_adaptive(const bdpt_frame_params* p, const bdpt_adaptive_params* a) {
    const std::string entry = "bdpt_render_adaptive: ";
    if (int rc = check_frame_size(p)) return rc;
    if (!a) return fail(BDPT_ERR_INVALID, entry + "null adaptive params");
    if (a->n_batches < 2 || a->n_batches > 64) return fail(BDPT_ERR_INVALID, entry + "n_batches must be in [2, 64]");
    if (a->step < 1) return fail(BDPT_ERR_INVALID, entry + "step must be >= 1");
    if (a->max_passes < 1 || a->max_passes > BDPT_ADAPTIVE_MAX_PASSES)
        return fail(BDPT_ERR_INVALID, entry + "max_passes" + in_range(BDPT_ADAPTIVE_MAX_PASSES));
    if (static_cast<int64_t>(a->max_passes) * a->step * a->n_batches != p->spp)
        return fail(BDPT_ERR_INVALID, entry + "spp must equal max_passes * step * n_batches (" + std::to_string(a->max_passes) +
                                          " * " + std::to_string(a->step) + " * " + std::to_string(a->n_batches) + "), got " +
                                          std::to_string(p->spp));
    if (!finite_nonneg(a->threshold)) return fail(BDPT_ERR_INVALID, entry + "threshold must be finite and >= 0");
    if (!finite_nonneg(a->eps)) return fail(BDPT_ERR_INVALID, entry + "eps must be finite and >= 0");
    if (a->dilate != 0 && a->dilate != 1) return fail(BDPT_ERR_INVALID, entry + "dilate must be 0 or 1");
    return BDPT_OK;
}

int bdpt_render_adaptive(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_adaptive_params* a, float* frame,
                         float* variance, int32_t* samples, bdpt_adaptive_stats* stats, void* hip_stream) {
    int rc = check_adaptive(p, a);
    if (rc) return rc;
    if (!c || !frame || !variance || !samples) return fail(BDPT_ERR_INVALID, "null argument");
    {  // what every pass's render would refuse, before anything is allocated or launched
        const Planes pl = pixel_planes(nullptr, 0);
        if ((rc = check_params(p)) || (rc = check_planes(c, p, pl)) || (rc = check_pixel_list(c, p, pl)) ||
            (rc = textured_frame_check(c, p)))
            return rc;
    }
    const int32_t W = p->width, H = p->height, K = a->n_batches, step = a->step;
    if (2ull * static_cast<uint64_t>(K) * static_cast<uint64_t>(W) * static_cast<uint64_t>(H) >= (1ull << 30))
        return fail(BDPT_ERR_INVALID, "bdpt_render_adaptive: 2 * n_batches * width * height must be below 2^30");
    const size_t N = static_cast<size_t>(W) * H, n = N * 3;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    HIP_TRY(c->ad_planes.reserve(sizeof(float) * 2 * n * K));
    HIP_TRY(c->ad_m.reserve(sizeof(int32_t) * N));
    HIP_TRY(c->ad_list.reserve(sizeof(int32_t) * N));
    HIP_TRY(c->ad_count.reserve(16));
    if ((rc = begin_use(c, st))) return rc;
    HIP_TRY(hipMemsetAsync(c->ad_planes, 0, sizeof(float) * 2 * n * K, st));
    HIP_TRY(launch_adaptive_start(N, step, c->ad_m, c->ad_list, st));
    if ((rc = end_use(c, st))) return rc;  // (the renders below order themselves after it)
    bdpt_adaptive_stats out{};
    c->ad_pass_lists.clear();
    int32_t count = static_cast<int32_t>(N);
    int64_t M = 0;  // the sum of m over the pixels: samples per batch traced so far
    for (int32_t j = 0; j < a->max_passes; j++) {
        for (int32_t b = 0; b < K; b++) {  // pass j, batch b: one window, into that batch's plane pair
            const bdpt_sample_window w = {j * step * K + b, K, step};
            if ((rc = render_bdpt(c, p, &w, c->ad_planes + static_cast<size_t>(b) * 2 * n, st, pixel_planes(c->ad_list, count))))
                return rc;
        }
        M += static_cast<int64_t>(count) * step;
        out.active[j] = count;
        out.passes = j + 1;
        if (a->record_passes) {
            const size_t at = c->ad_pass_lists.size();
            c->ad_pass_lists.resize(at + static_cast<size_t>(count));
            HIP_TRY(hipMemcpyAsync(c->ad_pass_lists.data() + at, c->ad_list, sizeof(int32_t) * static_cast<size_t>(count),
                                   hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        if (j + 1 == a->max_passes) break;  // the budget
        if ((rc = adaptive_resolve_launch(W, H, K, p->spp, c->ad_planes, c->ad_m, M, frame, variance, st))) return rc;
        if ((rc = adaptive_select_launch(c, W, H, frame, variance, a->threshold, a->eps, step, a->max_passes * step, a->dilate,
                                         c->ad_m, c->ad_list, c->ad_count, st)))
            return rc;
        HIP_TRY(hipMemcpyAsync(&count, c->ad_count, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (count < 0 || static_cast<size_t>(count) > N) return fail(BDPT_ERR_HIP, "bdpt_render_adaptive: a count outside [0, width * height]");
        if (count == 0) break;  // every pixel settled, or at its budget
    }
    out.samples = M * K;
    if ((rc = adaptive_resolve_launch(W, H, K, p->spp, c->ad_planes, c->ad_m, M, frame, variance, st))) return rc;
    HIP_TRY(launch_adaptive_samples(N, K, c->ad_m, samples, st));
    if ((rc = end_use(c, st))) return rc;
    if (stats) *stats = out;
    return BDPT_OK;
}

int bdpt_render_adaptive_host(bdpt_ctx* c, const bdpt_frame_params* p, const bdpt_adaptive_params* a, float* frame,
                              float* variance, int32_t* samples, bdpt_adaptive_stats* stats) {
    int rc = check_adaptive(p, a);
    if (rc) return rc;
    if (!c || !frame || !variance || !samples) return fail(BDPT_ERR_INVALID, "null argument");
    const size_t N = static_cast<size_t>(p->width) * p->height, n = N * 3;
    const size_t n16 = (n + 3) & ~static_cast<size_t>(3);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->ad_stage.reserve(2 * n16 * sizeof(float) + N * sizeof(int32_t)));
    float* const dframe = static_cast<float*>(c->ad_stage.get());
    float* const dvar = dframe + n16;
    int32_t* const dsamples = reinterpret_cast<int32_t*>(dvar + n16);
    if ((rc = bdpt_render_adaptive(c, p, a, dframe, dvar, dsamples, stats, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(frame, dframe, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(variance, dvar, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(samples, dsamples, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bdpt_stats bs;
    if ((rc = bdpt_get_stats(c, &bs))) return rc;
    if (bs.schedule_errors) return fail(BDPT_ERR_HIP, std::to_string(bs.schedule_errors) + " schedule errors");
    return BDPT_OK;
}

int bdpt_adaptive_pass_lists(bdpt_ctx* c, int32_t* out, int64_t capacity, int64_t* total) {
    if (!c || !total) return fail(BDPT_ERR_INVALID, "null argument");
    *total = static_cast<int64_t>(c->ad_pass_lists.size());
    if (!out) return BDPT_OK;
    if (capacity < *total) return fail(BDPT_ERR_INVALID, "bdpt_adaptive_pass_lists: capacity is below the lists' length");
    std::copy(c->ad_pass_lists.begin(), c->ad_pass_lists.end(), out);
    return BDPT_OK;
}

// ---------------------------------------------------------------- temporal accumulation
static int check_reproject(const bdpt_frame_params* p, const float* color, const float* aov, const float* hist_in,
                           const float* out, const float* hist_out, const bdpt_reproject_params* r) {
    const std::string entry = "bdpt_reproject: ";
    if (!p) return fail(BDPT_ERR_INVALID, entry + "null frame params");
    if (!r) return fail(BDPT_ERR_INVALID, entry + "null reproject params");
    if (p->width <= 0 || p->height <= 0) return fail(BDPT_ERR_INVALID, entry + "width/height must be > 0");
    const uint64_t px = static_cast<uint64_t>(p->width) * static_cast<uint64_t>(p->height);
    if (px >= (1ull << 28)) return fail(BDPT_ERR_INVALID, entry + "width * height must be below 2^28");
    auto positive = [](float v) { return v > 0.f && std::isfinite(v); };
    if (!positive(r->norm)) return fail(BDPT_ERR_INVALID, entry + "norm must be > 0");
    if (!positive(r->cur_samples)) return fail(BDPT_ERR_INVALID, entry + "cur_samples must be > 0");
    if (!positive(r->max_history)) return fail(BDPT_ERR_INVALID, entry + "max_history must be > 0");
    if (!positive(r->sigma_normal)) return fail(BDPT_ERR_INVALID, entry + "sigma_normal must be > 0");
    if (!positive(r->sigma_depth)) return fail(BDPT_ERR_INVALID, entry + "sigma_depth must be > 0");
    if (!(r->min_weight > 0.f && r->min_weight <= 1.f)) return fail(BDPT_ERR_INVALID, entry + "min_weight must be in (0, 1]");
    if (!(r->clamp_sigma >= 0.f) || !std::isfinite(r->clamp_sigma)) return fail(BDPT_ERR_INVALID, entry + "clamp_sigma must be >= 0");
    if (r->demodulate != 0 && r->demodulate != 1) return fail(BDPT_ERR_INVALID, entry + "demodulate must be 0 or 1");
    if (!color) return fail(BDPT_ERR_INVALID, entry + "color must not be NULL");
    if (!aov) return fail(BDPT_ERR_INVALID, entry + "aov must not be NULL");
    if (!out) return fail(BDPT_ERR_INVALID, entry + "out_color must not be NULL");
    if (!hist_out) return fail(BDPT_ERR_INVALID, entry + "hist_out must not be NULL");
    const FloatSpan in[] = {{"color", color, px * 3}, {"aov", aov, px * 8}, {"hist_in", hist_in, px * 8}};
    const FloatSpan outs[] = {{"out_color", out, px * 3}, {"hist_out", hist_out, px * 8}};
    for (const FloatSpan& o : outs)
        for (const FloatSpan& i : in)
            if (spans_overlap(o, i)) return fail(BDPT_ERR_INVALID, entry + o.name + " overlaps " + i.name);
    if (spans_overlap(outs[1], outs[0])) return fail(BDPT_ERR_INVALID, entry + "hist_out overlaps out_color");
    return BDPT_OK;
}

int bdpt_reproject(bdpt_ctx* c, const bdpt_frame_params* p, const float* color, const float* aov, const float* hist_in,
                   float* out, float* hist_out, const bdpt_reproject_params* r, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_reproject(p, color, aov, hist_in, out, hist_out, r);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    // the current camera's frame as camera_dir reads it: camera, size, and spp 1 (the pixel centre, no draws)
    dev::DevFrame fr{};
    camera_constants(p->camera.eye, p->camera.at, p->camera.up, p->camera.fov, p->width, p->height, fr.cam);
    fr.W = p->width, fr.H = p->height, fr.spp = 1;
    CameraConstants prev;
    const bdpt_camera& pc = r->prev_camera;
    camera_constants(pc.eye, pc.at, pc.up, pc.fov, p->width, p->height, prev);
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    HIP_TRY(launch_reproject(fr, prev, r->norm, r->cur_samples, r->max_history, r->sigma_normal, r->sigma_depth,
                             r->min_weight, r->clamp_sigma, r->demodulate, color, aov, hist_in, out, hist_out, st));
    return end_timed(c, st, 0, 1);
}

int bdpt_reproject_host(bdpt_ctx* c, const bdpt_frame_params* p, const float* color, const float* aov,
                        const float* hist_in, float* out, float* hist_out, const bdpt_reproject_params* r) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_reproject(p, color, aov, hist_in, out, hist_out, r);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = static_cast<size_t>(p->width) * p->height;
    HIP_TRY(c->tmp_fb.reserve(px * 30 * sizeof(float)));
    // aov, hist_in, hist_out (each a multiple of 32 bytes from the 16-byte aligned start), color, out_color
    float *da = c->tmp_fb, *dhi = da + px * 8, *dho = da + px * 16, *dc = da + px * 24, *dout = da + px * 27;
    HIP_TRY(hipMemcpyAsync(da, aov, px * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dc, color, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (hist_in) HIP_TRY(hipMemcpyAsync(dhi, hist_in, px * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_reproject(c, p, dc, da, hist_in ? dhi : nullptr, dout, dho, r, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hist_out, dho, px * 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// ---------------------------------------------------------------- display output
// The encode's curve in double, on y >= 0.
static double encode_curve(int32_t encode, double y) {
    if (encode == BDPT_ENCODE_SRGB) return y <= 0.0031308 ? 12.92 * y : 1.055 * std::pow(y, 1.0 / 2.4) - 0.055;
    if (encode == BDPT_ENCODE_GAMMA22) return std::pow(y, 1.0 / 2.2);
    return y;
}

int bdpt_display_thresholds(int32_t encode, float out[255]) {
    if (encode != BDPT_ENCODE_SRGB && encode != BDPT_ENCODE_GAMMA22 && encode != BDPT_ENCODE_LINEAR)
        return fail(BDPT_ERR_INVALID, "bdpt_display_thresholds: encode must be BDPT_ENCODE_SRGB, _GAMMA22 or _LINEAR");
    if (!out) return fail(BDPT_ERR_INVALID, "bdpt_display_thresholds: out must not be NULL");
    for (int k = 1; k <= 255; k++) {
        const double target = (k - 0.5) / 255.0;
        // a start near the step from the inverse curve, then float by float to the smallest t that reaches it
        double y = target;
        if (encode == BDPT_ENCODE_SRGB) y = target <= 12.92 * 0.0031308 ? target / 12.92 : std::pow((target + 0.055) / 1.055, 2.4);
        else if (encode == BDPT_ENCODE_GAMMA22) y = std::pow(target, 2.2);
        float t = static_cast<float>(y);
        while (encode_curve(encode, t) < target) t = std::nextafterf(t, 2.f);
        for (float below = std::nextafterf(t, 0.f); t > 0.f && encode_curve(encode, below) >= target; below = std::nextafterf(t, 0.f)) t = below;
        out[k - 1] = t;
    }
    return BDPT_OK;
}

struct ByteSpan {
    const char* name;
    const void* p;
    size_t bytes;
};
static bool byte_spans_overlap(const ByteSpan& a, const ByteSpan& b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a.p && b.p && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
static int check_image_size(const std::string& entry, int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return fail(BDPT_ERR_INVALID, entry + "width/height must be > 0");
    if (static_cast<uint64_t>(width) * static_cast<uint64_t>(height) >= (1ull << 28))
        return fail(BDPT_ERR_INVALID, entry + "width * height must be below 2^28");
    return BDPT_OK;
}
static bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

static int check_meter(int32_t width, int32_t height, const float* color, const float* aov, const uint32_t* prev,
                       const bdpt_meter_params* m, const uint32_t* out) {
    const std::string entry = "bdpt_meter: ";
    if (!m) return fail(BDPT_ERR_INVALID, entry + "null meter params");
    if (int rc = check_image_size(entry, width, height)) return rc;
    if (!positive_finite(m->norm)) return fail(BDPT_ERR_INVALID, entry + "norm must be > 0");
    if (!positive_finite(m->key)) return fail(BDPT_ERR_INVALID, entry + "key must be > 0");
    if (m->key_permille < 1 || m->key_permille > 1000) return fail(BDPT_ERR_INVALID, entry + "key_permille must be in [1, 1000]");
    if (m->white_permille < 1 || m->white_permille > 1000) return fail(BDPT_ERR_INVALID, entry + "white_permille must be in [1, 1000]");
    if (!(m->rate > 0.f && m->rate <= 1.f)) return fail(BDPT_ERR_INVALID, entry + "rate must be in (0, 1]");
    if (!positive_finite(m->fallback_exposure)) return fail(BDPT_ERR_INVALID, entry + "fallback_exposure must be > 0");
    if (!positive_finite(m->fallback_white)) return fail(BDPT_ERR_INVALID, entry + "fallback_white must be > 0");
    if (!color) return fail(BDPT_ERR_INVALID, entry + "color must not be NULL");
    if (!out) return fail(BDPT_ERR_INVALID, entry + "out_words must not be NULL");
    const size_t px = static_cast<size_t>(width) * height;
    const ByteSpan o = {"out_words", out, 16};
    const ByteSpan in[] = {{"color", color, px * 12}, {"aov", aov, px * 32}, {"prev", prev, 16}};
    for (const ByteSpan& i : in)
        if (byte_spans_overlap(o, i)) return fail(BDPT_ERR_INVALID, entry + o.name + " overlaps " + i.name);
    return BDPT_OK;
}

int bdpt_meter(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const float* aov, const uint32_t* prev,
               const bdpt_meter_params* m, uint32_t* out, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_meter(width, height, color, aov, prev, m, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    HIP_TRY(c->meter_hist.reserve(sizeof(uint32_t) * BDPT_METER_BINS));
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    HIP_TRY(launch_meter(color, aov, prev, m->norm, m->key, m->key_permille, m->white_permille, m->rate, m->fallback_exposure,
                         m->fallback_white, static_cast<size_t>(width) * height, c->meter_hist, out, st));
    return end_timed(c, st, 0, 2);
}

// The host forms' staging: [16-byte aligned parts] color, aov, 4 words in, 4 words out, display bytes.
static size_t up16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

int bdpt_meter_host(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const float* aov, const uint32_t* prev,
                    const bdpt_meter_params* m, uint32_t out[4]) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_meter(width, height, color, aov, prev, m, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = static_cast<size_t>(width) * height, nc = up16(px * 12), na = up16(px * 32);
    HIP_TRY(c->display_stage.reserve(nc + na + 32));
    char* const base = static_cast<char*>(c->display_stage.get());
    float* const dc = reinterpret_cast<float*>(base);
    float* const da = reinterpret_cast<float*>(base + nc);
    uint32_t* const dprev = reinterpret_cast<uint32_t*>(base + nc + na);
    uint32_t* const dout = dprev + 4;
    HIP_TRY(hipMemcpyAsync(dc, color, px * 12, hipMemcpyHostToDevice, c->stream));
    if (aov) HIP_TRY(hipMemcpyAsync(da, aov, px * 32, hipMemcpyHostToDevice, c->stream));
    if (prev) HIP_TRY(hipMemcpyAsync(dprev, prev, 16, hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_meter(c, width, height, dc, aov ? da : nullptr, prev ? dprev : nullptr, m, dout, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_debug_meter_histogram(bdpt_ctx* c, uint32_t out[BDPT_METER_BINS]) {
    if (!c || !out) return fail(BDPT_ERR_INVALID, "null argument");
    if (!c->meter_hist.get()) return fail(BDPT_ERR_INVALID, "bdpt_debug_meter_histogram: no bdpt_meter call on this context yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->meter_hist, sizeof(uint32_t) * BDPT_METER_BINS, hipMemcpyDeviceToHost));
    return BDPT_OK;
}

static int check_display(int32_t width, int32_t height, const float* color, const uint32_t* meter,
                         const bdpt_display_params* d, const unsigned char* out) {
    const std::string entry = "bdpt_display: ";
    if (!d) return fail(BDPT_ERR_INVALID, entry + "null display params");
    if (int rc = check_image_size(entry, width, height)) return rc;
    if (!positive_finite(d->norm)) return fail(BDPT_ERR_INVALID, entry + "norm must be > 0");
    if (!positive_finite(d->exposure)) return fail(BDPT_ERR_INVALID, entry + "exposure must be > 0");
    if (!positive_finite(d->white)) return fail(BDPT_ERR_INVALID, entry + "white must be > 0");
    if (d->tone != BDPT_TONE_CLAMP && d->tone != BDPT_TONE_REINHARD && d->tone != BDPT_TONE_FILMIC)
        return fail(BDPT_ERR_INVALID, entry + "tone must be BDPT_TONE_CLAMP, _REINHARD or _FILMIC");
    if (d->encode != BDPT_ENCODE_SRGB && d->encode != BDPT_ENCODE_GAMMA22 && d->encode != BDPT_ENCODE_LINEAR)
        return fail(BDPT_ERR_INVALID, entry + "encode must be BDPT_ENCODE_SRGB, _GAMMA22 or _LINEAR");
    if (d->channels != 3 && d->channels != 4) return fail(BDPT_ERR_INVALID, entry + "channels must be 3 or 4");
    if (!color) return fail(BDPT_ERR_INVALID, entry + "color must not be NULL");
    if (!out) return fail(BDPT_ERR_INVALID, entry + "out must not be NULL");
    const size_t px = static_cast<size_t>(width) * height;
    const ByteSpan o = {"out", out, px * static_cast<size_t>(d->channels)};
    const ByteSpan in[] = {{"color", color, px * 12}, {"meter", meter, 16}};
    for (const ByteSpan& i : in)
        if (byte_spans_overlap(o, i)) return fail(BDPT_ERR_INVALID, entry + o.name + " overlaps " + i.name);
    return BDPT_OK;
}

int bdpt_display(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const uint32_t* meter,
                 const bdpt_display_params* d, unsigned char* out, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_display(width, height, color, meter, d, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if (!c->display_tables_ready) {  // once per context: the three tables, 256 floats apart
        float host[3 * 256] = {};
        for (int32_t enc = 0; enc < 3; enc++)
            if ((rc = bdpt_display_thresholds(enc, host + 256 * enc))) return rc;
        HIP_TRY(c->display_tables.reserve(sizeof(host)));
        HIP_TRY(hipMemcpy(c->display_tables, host, sizeof(host), hipMemcpyHostToDevice));
        c->display_tables_ready = true;
    }
    if ((rc = begin_use(c, st))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    HIP_TRY(launch_display(color, c->display_tables.get() + 256 * d->encode, meter, d->norm, d->exposure, d->white, d->tone,
                           d->channels, static_cast<size_t>(width) * height, out, st));
    return end_timed(c, st, 0, 1);
}

int bdpt_display_host(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const uint32_t* meter,
                      const bdpt_display_params* d, unsigned char* out) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_display(width, height, color, meter, d, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = static_cast<size_t>(width) * height, nc = up16(px * 12), nb = px * static_cast<size_t>(d->channels);
    HIP_TRY(c->display_stage.reserve(nc + 16 + nb));
    char* const base = static_cast<char*>(c->display_stage.get());
    float* const dc = reinterpret_cast<float*>(base);
    uint32_t* const dmeter = reinterpret_cast<uint32_t*>(base + nc);
    unsigned char* const dout = reinterpret_cast<unsigned char*>(base + nc + 16);
    HIP_TRY(hipMemcpyAsync(dc, color, px * 12, hipMemcpyHostToDevice, c->stream));
    if (meter) HIP_TRY(hipMemcpyAsync(dmeter, meter, 16, hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_display(c, width, height, dc, meter ? dmeter : nullptr, d, dout, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

static int check_denoise_var(int32_t width, int32_t height, const float* color, const float* var, const float* aov,
                             const float* out, const float* out_var, const bdpt_denoise_params* d) {
    const std::string entry = "bdpt_denoise_var";
    if (!color || !aov || !out || !d) return fail(BDPT_ERR_INVALID, "null argument");
    if (!var) return fail(BDPT_ERR_INVALID, entry + ": var must not be NULL");
    if (int rc = check_denoise_fields(entry, width, height, d)) return rc;
    const size_t px = static_cast<size_t>(width) * height;
    const FloatSpan in[] = {{"color", color, px * 3}, {"var", var, px * 3}, {"aov", aov, px * 8}};
    const FloatSpan outs[] = {{"out", out, px * 3}, {"out_var", out_var, px}};
    for (const FloatSpan& o : outs)
        for (const FloatSpan& i : in)
            if (spans_overlap(o, i)) return fail(BDPT_ERR_INVALID, entry + ": " + o.name + " overlaps " + i.name);
    if (spans_overlap(outs[1], outs[0])) return fail(BDPT_ERR_INVALID, entry + ": out_var overlaps out");
    return BDPT_OK;
}

int bdpt_denoise_var(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const float* var, const float* aov,
                     float* out, float* out_var, const bdpt_denoise_params* d, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_denoise_var(width, height, color, var, aov, out, out_var, d);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t px = static_cast<size_t>(width) * height;
    const int it = d->iterations;
    if ((rc = begin_use(c, st))) return rc;
    if ((it > 0 || out_var) && (rc = reserve_denoise_scratch(c, px))) return rc;
    if ((rc = begin_timed(c, st))) return rc;
    if (it == 0) {
        HIP_TRY(launch_denoise_scale(px * 3, color, d->norm, out, st));
        if (!out_var) return end_timed(c, st, 0, 1);
    }
    // (I_0, U) in image 0, (I_0, V_0) in image 1; iteration i then reads image (i + 1) & 1 and writes image i & 1
    HIP_TRY(launch_denoise_var_prepare(width, height, color, var, aov, d->norm, d->demodulate, c->dn_guide, c->dn_img[0], st));
    HIP_TRY(launch_denoise_var_blur(width, height, c->dn_img[0], c->dn_img[1], it == 0 ? out_var : nullptr, st));
    const float sc2 = d->sigma_color * d->sigma_color, inv_n = 1.f / (d->sigma_normal * d->sigma_normal);
    for (int i = 0; i < it; i++)
        HIP_TRY(launch_denoise_var_iter(width, height, 1 << i, sc2, inv_n, d->sigma_depth, d->demodulate, c->dn_guide,
                                        c->dn_img[(i + 1) & 1], c->dn_img[i & 1], out, out_var, i + 1 == it, st));
    return end_timed(c, st, 0, it == 0 ? 3 : it + 2);
}

int bdpt_denoise_var_host(bdpt_ctx* c, int32_t width, int32_t height, const float* color, const float* var,
                          const float* aov, float* out, float* out_var, const bdpt_denoise_params* d) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_denoise_var(width, height, color, var, aov, out, out_var, d);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = static_cast<size_t>(width) * height;
    HIP_TRY(c->tmp_fb.reserve(px * 18 * sizeof(float)));
    // color, var, aov, out, out_var (16-byte aligned or not: scalar loads and stores)
    float *dc = c->tmp_fb, *dv = dc + px * 3, *da = dv + px * 3, *dout = da + px * 8, *dov = dout + px * 3;
    HIP_TRY(hipMemcpyAsync(dc, color, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dv, var, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(da, aov, px * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_denoise_var(c, width, height, dc, dv, da, dout, out_var ? dov : nullptr, d, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_var) HIP_TRY(hipMemcpyAsync(out_var, dov, px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// OWN mode filters frames of up to this many pixels in chunks and larger ones plane by plane: measured
// (DESIGN.md §7h), the chunks are 1.4 to 1.8 x the loop at 512^2 and 0.91 to 1.05 x at 1024^2.
constexpr size_t kDenoisePlanesOwnChunkPixels = 512 * 512;

static int check_denoise_planes(int32_t width, int32_t height, int32_t n_planes, const float* planes, const float* aov,
                                const float* guide_color, int32_t mode, const bdpt_denoise_params* d,
                                const float* out_planes, const float* out_guide) {
    const std::string entry = "bdpt_denoise_planes";
    if (!planes || !aov || !out_planes || !d) return fail(BDPT_ERR_INVALID, "null argument");
    if (int rc = check_denoise_fields(entry, width, height, d)) return rc;
    if (n_planes < 1) return fail(BDPT_ERR_INVALID, entry + ": n_planes must be >= 1");
    const size_t px = static_cast<size_t>(width) * height;
    if (static_cast<uint64_t>(n_planes) * px >= (1ull << 30))
        return fail(BDPT_ERR_INVALID, entry + ": n_planes * width * height must be below 2^30");
    if (mode != BDPT_DENOISE_PLANES_OWN && mode != BDPT_DENOISE_PLANES_SHARED)
        return fail(BDPT_ERR_INVALID, entry + ": mode must be BDPT_DENOISE_PLANES_OWN or BDPT_DENOISE_PLANES_SHARED");
    if (mode == BDPT_DENOISE_PLANES_OWN && guide_color)
        return fail(BDPT_ERR_INVALID, entry + ": guide_color must be NULL in OWN mode");
    if (mode == BDPT_DENOISE_PLANES_OWN && out_guide)
        return fail(BDPT_ERR_INVALID, entry + ": out_guide must be NULL in OWN mode");
    struct Span {
        const char* name;
        const float* p;
        size_t floats;
    };
    const Span in[] = {{"planes", planes, n_planes * px * 3}, {"aov", aov, px * 8}, {"guide_color", guide_color, px * 3}};
    const Span outs[] = {{"out_planes", out_planes, n_planes * px * 3}, {"out_guide", out_guide, px * 3}};
    auto overlap = [](const Span& a, const Span& b) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
        return a.p && b.p && a0 < b0 + b.floats * sizeof(float) && b0 < a0 + a.floats * sizeof(float);
    };
    for (const Span& o : outs)
        for (const Span& i : in)
            if (overlap(o, i)) return fail(BDPT_ERR_INVALID, entry + ": " + o.name + " overlaps " + i.name);
    if (overlap(outs[1], outs[0])) return fail(BDPT_ERR_INVALID, entry + ": out_guide overlaps out_planes");
    return BDPT_OK;
}

int bdpt_denoise_planes(bdpt_ctx* c, int32_t width, int32_t height, int32_t n_planes, const float* planes,
                        const float* aov, const float* guide_color, int32_t mode, const bdpt_denoise_params* d,
                        float* out_planes, float* out_guide, void* hip_stream) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_denoise_planes(width, height, n_planes, planes, aov, guide_color, mode, d, out_planes, out_guide);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t px = static_cast<size_t>(width) * height, plane = px * 3;
    const bool shared = mode == BDPT_DENOISE_PLANES_SHARED;
    const int P = denoise_planes_chunk(), it = d->iterations;
    if ((rc = begin_use(c, st))) return rc;
    if (it > 0) {
        HIP_TRY(c->dnp_guide.reserve(px * 32));
        if (shared) HIP_TRY(c->dnp_traj.reserve(px * 16 * 8));
        HIP_TRY(c->dnp_img[0].reserve(px * 16 * P));
        HIP_TRY(c->dnp_img[1].reserve(px * 16 * P));
    }
    if ((rc = begin_timed(c, st))) return rc;
    int64_t launches = 0;
    if (it == 0) {
        HIP_TRY(launch_denoise_scale(plane * n_planes, planes, d->norm, out_planes, st));
        launches++;
        if (out_guide) {
            if (guide_color) HIP_TRY(launch_denoise_scale(plane, guide_color, d->norm, out_guide, st));
            else HIP_TRY(launch_planes_sum(planes, plane, n_planes, d->norm, out_guide, st));
            launches++;
        }
        return end_timed(c, st, 0, launches);
    }
    // sigma_color of iteration i, squared and inverted as bdpt_denoise does
    auto inv_c = [&](int i) {
        const float sc_i = d->sigma_color * std::ldexp(1.f, -i);
        return 1.f / (sc_i * sc_i);
    };
    const float inv_n = 1.f / (d->sigma_normal * d->sigma_normal);
    float4* const traj = static_cast<float4*>(c->dnp_traj.get());  // B_i at traj + i * px
    if (shared) {
        // The guides and the guide's own filter, with bdpt_denoise's kernels: B_0 .. B_{it-1} stay in traj, the
        // last update goes to out_guide if anyone wants it. A summed G waits in B_1's place until B_0 is formed.
        const float* g = guide_color;
        if (!g) {
            float* sum = reinterpret_cast<float*>(traj + px);
            HIP_TRY(launch_planes_sum(planes, plane, n_planes, 1.f, sum, st));
            launches++;
            g = sum;
        }
        HIP_TRY(launch_denoise_prepare(width, height, g, aov, d->norm, d->demodulate, c->dnp_guide, traj, st));
        const int guide_its = out_guide ? it : it - 1;
        for (int i = 0; i < guide_its; i++)
            HIP_TRY(launch_denoise_iter(width, height, 1 << i, inv_c(i), inv_n, d->sigma_depth, d->demodulate, c->dnp_guide,
                                        traj + i * px, traj + (i + 1 < it ? i + 1 : 0) * px, out_guide, i + 1 == it, st));
        launches += 1 + guide_its;
    } else if (px > kDenoisePlanesOwnChunkPixels) {
        // a large frame: bdpt_denoise's launches per plane, which the chunks do not beat there
        for (int j = 0; j < n_planes; j++) {
            HIP_TRY(launch_denoise_prepare(width, height, planes + j * plane, aov, d->norm, d->demodulate, c->dnp_guide,
                                           c->dnp_img[0], st));
            for (int i = 0; i < it; i++)
                HIP_TRY(launch_denoise_iter(width, height, 1 << i, inv_c(i), inv_n, d->sigma_depth, d->demodulate,
                                            c->dnp_guide, c->dnp_img[i & 1], c->dnp_img[(i + 1) & 1], out_planes + j * plane,
                                            i + 1 == it, st));
        }
        return end_timed(c, st, 0, static_cast<int64_t>(n_planes) * (1 + it));
    } else {
        // only the packed guides are wanted; the image this writes is overwritten by the first chunk
        HIP_TRY(launch_denoise_prepare(width, height, planes, aov, d->norm, d->demodulate, c->dnp_guide, c->dnp_img[0], st));
        launches++;
    }
    for (int first = 0; first < n_planes; first += P) {
        const int cnt = std::min(P, n_planes - first);
        HIP_TRY(launch_denoise_planes_prepare(width, height, planes + first * plane, cnt, d->norm, d->demodulate,
                                              c->dnp_guide, c->dnp_img[0], st));
        for (int i = 0; i < it; i++)
            HIP_TRY(launch_denoise_planes_iter(width, height, 1 << i, inv_c(i), inv_n, d->sigma_depth, d->demodulate, cnt,
                                               c->dnp_guide, shared ? traj + i * px : nullptr, c->dnp_img[i & 1],
                                               c->dnp_img[(i + 1) & 1], out_planes + first * plane, i + 1 == it, st));
        launches += 1 + it;
    }
    return end_timed(c, st, 0, launches);
}

int bdpt_denoise_planes_host(bdpt_ctx* c, int32_t width, int32_t height, int32_t n_planes, const float* planes,
                             const float* aov, const float* guide_color, int32_t mode, const bdpt_denoise_params* d,
                             float* out_planes, float* out_guide) {
    if (!c) return fail(BDPT_ERR_INVALID, "null ctx");
    int rc = check_denoise_planes(width, height, n_planes, planes, aov, guide_color, mode, d, out_planes, out_guide);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = static_cast<size_t>(width) * height, all = px * 3 * n_planes;
    HIP_TRY(c->tmp_fb.reserve((2 * all + px * 14) * sizeof(float)));
    // planes, out_planes, aov, guide_color, out_guide (16-byte aligned or not: scalar loads and stores)
    float *dp = c->tmp_fb, *dout = dp + all, *da = dout + all, *dg = da + px * 8, *dog = dg + px * 3;
    HIP_TRY(hipMemcpyAsync(dp, planes, all * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(da, aov, px * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (guide_color) HIP_TRY(hipMemcpyAsync(dg, guide_color, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = bdpt_denoise_planes(c, width, height, n_planes, dp, da, guide_color ? dg : nullptr, mode, d, dout,
                                  out_guide ? dog : nullptr, c->stream)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out_planes, dout, all * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_guide) HIP_TRY(hipMemcpyAsync(out_guide, dog, px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_splat_to_image_plane(bdpt_ctx* c, const bdpt_frame_params* p, int64_t n, const float* pts, int32_t* xy) {
    if (!c || !p || n < 0 || (n > 0 && (!pts || !xy))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (p->width <= 0 || p->height <= 0) return fail(BDPT_ERR_INVALID, "width/height must be > 0");
    if (n == 0) return BDPT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = begin_use(c, c->stream))) return rc;
    DevBuf<float> dp;
    DevBuf<int32_t> dxy;
    const size_t N = static_cast<size_t>(n);
    if ((rc = kat_in(c, dp, pts, 12 * N)) || (rc = kat_in<int32_t>(c, dxy, nullptr, 8 * N))) return rc;
    HIP_TRY(launch_splat_kat(make_frame(p), n, dp, dxy, c->stream));
    HIP_TRY(hipMemcpyAsync(xy, dxy, 8 * N, hipMemcpyDeviceToHost, c->stream));
    if ((rc = end_use(c, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_debug_sampling(bdpt_ctx* c, const bdpt_frame_params* p, int32_t build, int32_t fn, int32_t placement,
                        int64_t n, const void* in, void* out, int32_t* ctx_placement) {
    static const int kIn[] = {1, 2, 2, 2, 9, 12, 2, 4, 3}, kOut[] = {1, 3, 2, 3, 4, 1, 1, 10, 3};
    if (!c || n < 0 || (n > 0 && (!in || !out))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (ctx_placement) *ctx_placement = c->sc.lds_etri_off != dev::kNoLds ? BDPT_EMITTERS_LDS : BDPT_EMITTERS_HBM;
    if (build != BDPT_KAT_EXACT && build != BDPT_KAT_FAST)
        return fail(BDPT_ERR_INVALID, "bdpt_debug_sampling: build must be BDPT_KAT_EXACT or BDPT_KAT_FAST");
    if (fn < BDPT_SAMPLING_CANONICAL || fn > BDPT_SAMPLING_CAMERA) return fail(BDPT_ERR_INVALID, "bad function code");
    if (placement < BDPT_EMITTERS_CTX || placement > BDPT_EMITTERS_LDS) return fail(BDPT_ERR_INVALID, "bad placement");
    dev::DevFrame fr{};
    if (fn == BDPT_SAMPLING_CAMERA) {
        if (int rc = check_frame_size(p)) return rc;
        if (int rc = check_row_shard(p)) return rc;
        fr = make_frame(p);
    }
    dev::DevScene sc = c->sc;
    if (placement == BDPT_EMITTERS_HBM) {
        sc.lds_etri_off = sc.lds_ecdf_off = dev::kNoLds;
        sc.lds_words = c->lds_words_base;
    } else if (placement == BDPT_EMITTERS_LDS) {
        const uint32_t with = emitter_lds_layout(sc, c->lds_words_base, sc.lds_etri_off, sc.lds_ecdf_off);
        if (with * 4ull > kLdsBudget)
            return fail(BDPT_ERR_UNSUPPORTED, "bdpt_debug_sampling: the emitter faces and CDFs (" +
                                                  std::to_string(with * 4ull) + " bytes with the other tables) "
                                                  "exceed the 24 KiB LDS budget");
        sc.lds_words = with;
    }
    const uint32_t* win = static_cast<const uint32_t*>(in);
    if (fn == BDPT_SAMPLING_CDF)
        for (int64_t i = 0; i < n; i++)
            if (win[2 * i] >= static_cast<uint32_t>(c->sc.nemit)) return fail(BDPT_ERR_INVALID, "emitter index out of range");
    if (n == 0) return BDPT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = begin_use(c, c->stream))) return rc;
    DevBuf<uint32_t> din, dout;
    const size_t N = static_cast<size_t>(n), bi = 4 * N * kIn[fn], bo = 4 * N * kOut[fn];
    if ((rc = kat_in(c, din, win, bi)) || (rc = kat_in<uint32_t>(c, dout, nullptr, bo))) return rc;
    const auto launch = build == BDPT_KAT_FAST ? launch_sampling_kat_fw : launch_sampling_kat;
    HIP_TRY(launch(sc, fr, fn, kIn[fn], kOut[fn], n, din, dout, c->stream));
    HIP_TRY(hipMemcpyAsync(out, dout, bo, hipMemcpyDeviceToHost, c->stream));
    if ((rc = end_use(c, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// Device-only diagnostics without a scene (synchronous, default stream).
static int device_kat(int32_t device, size_t in_bytes, const float* in, size_t in2_bytes, const float* in2,
                      size_t out_bytes, float* out,
                      hipError_t (*launch)(const float*, const float*, float*)) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(BDPT_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(BDPT_ERR_INVALID, "bad device");
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> a, b, o;
    hipError_t e = a.reserve(std::max<size_t>(in_bytes, 16));
    if (e == hipSuccess) e = b.reserve(std::max<size_t>(in2_bytes, 16));
    if (e == hipSuccess) e = o.reserve(std::max<size_t>(out_bytes, 16));
    if (e == hipSuccess) e = hipMemcpy(a, in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && in2) e = hipMemcpy(b, in2, in2_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch(a, b, o);
    if (e == hipSuccess) e = hipMemcpy(out, o, out_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(BDPT_ERR_HIP, std::string("device diagnostic: ") + hipGetErrorString(e));
    return BDPT_OK;
}

static thread_local int64_t g_kat_n = 0;

int bdpt_debug_fresnel(int32_t device, int64_t n, const float* in, float* out) {
    if (n < 0 || (n > 0 && (!in || !out))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (n == 0) return BDPT_OK;
    g_kat_n = n;
    const size_t N = static_cast<size_t>(n);
    return device_kat(device, 16 * N, in, 0, nullptr, 4 * N, out, [](const float* a, const float*, float* o) {
        return launch_fresnel_kat(g_kat_n, a, o, nullptr);
    });
}

int bdpt_debug_triangle(int32_t device, int64_t n, const float* rays, const float* verts, float* out) {
    if (n < 0 || (n > 0 && (!rays || !verts || !out))) return fail(BDPT_ERR_INVALID, "bad argument");
    if (n == 0) return BDPT_OK;
    g_kat_n = n;
    const size_t N = static_cast<size_t>(n);
    return device_kat(device, 32 * N, rays, 36 * N, verts, 16 * N, out, [](const float* a, const float* b, float* o) {
        return launch_triangle_kat(g_kat_n, a, b, o, nullptr);
    });
}

}  // extern "C"

// tinyrender_amd — the reference's command line (src/main.cpp:121-181,
// `tinyrender <scene.toml> [nogui]`) for the BDPT path on an MI355X:
// loadTOML -> Scene::load -> Integrator::init -> the timed render
// (main.cpp:146-152, "Render took: ... seconds.") -> Integrator::save, which
// writes the EXR next to the TOML (integrator.cpp:26-30).
//
// Offline `type = "bdpt"` (the hot path), `type = "path"` and `type = "direct"`
// (the reference's PathTracerIntegrator and DirectIntegrator on the same
// substrate) are accepted; the other
// integrators and the realtime render passes are rejected with an error.
// Optional overrides (not in the reference): --width W --height H --spp N
// --rr D --device K --out FILE.exr --seed S, and --gpus N / --devices a,b,...
// to render on several devices (row shards + one RCCL sum-reduce, bdpt_multi_*);
// --shard samples|rows picks how those devices split the frame
// (bdpt_multi_set_sharding), and --sample-window F:S:C renders only the samples
// F, F + S, ... (C of them) of every pixel and writes that partial image
// (bdpt_render_window_host; partial images of windows that partition the spp sum
// to the frame). A malformed or out-of-range window is refused before any device is used.
// --aov also writes <out>_albedo.exr and <out>_normal.exr (the first-hit feature buffers of
// bdpt_render_aov_host, 3 channels each, divided by the coverage), --denoise[=ITER] also
// <out>_denoised.exr (bdpt_denoise_host with the header's defaults, ITER iterations 0..8);
// the main EXR is the same bytes with or without them. Both combine with --sample-window
// (the filter's norm is spp / count); with several devices the first one renders the
// feature buffers and filters the reduced frame.
// --layers N (1..64, a bdpt scene) also writes <out stem>.L00.exr ... .L<N-1>.exr, the frame split
// by path length (bdpt_render_layers_host: layer l holds the paths of l + 1 edges, the last one
// everything longer; a second render, so the main EXR is the same bytes with or without it). A
// malformed N is refused before any device is used; with several devices the first renders them.
// --light-groups (a bdpt scene of at most 64 emitters) also writes <out stem>.E00.exr ..., the frame
// split by emitter under the identity map (bdpt_render_light_groups_host: file e holds the paths
// that end on emitter e of bdpt_scene_get_emitter; a second render, so the main EXR is the same
// bytes with or without it). Refused for path / direct scenes before any device is used; with
// several devices the first renders the groups.
// --strategies[=unweighted] (a bdpt scene) also writes <out stem>.S<ss>T<tt>.exr for every plane of
// the frame split by sampling strategy that is not all zero (bdpt_render_strategies_host at
// bdpt_strategies_shape's shape: s light-subpath and t eye-subpath vertices; =unweighted: without the
// MIS weights) and <out stem>.strategies.exr, their contact sheet at gain 1 (bdpt_strategies_sheet).
// A second render, so the main EXR is the same bytes with or without it. A bad value, a path / direct
// scene or an rr_depth outside 1..28 is refused before any device is used; with several devices the
// first renders the planes.
// --cross (with --light-groups and exactly one of --layers N / --strategies[=unweighted]) writes the
// product of the two splits instead of the two sets of files: <out stem>.E<ee>L<ll>.exr, a plane per
// (emitter, layer) (bdpt_render_group_layers_host), or <out stem>.E<ee>S<ss>T<tt>.exr for every
// (emitter, s, t) plane that is not all zero (bdpt_render_group_strategies_host; no contact sheet).
// Without --cross the two flags keep writing their two independent sets. Refusals and devices as for
// the single flags.
// --denoise-planes[=own|shared] (default shared; with at least one of the plane flags above) filters
// every plane set those flags write with bdpt_denoise_planes_host (the header's defaults, --denoise=ITER's
// iteration count if that flag is given too) and writes, next to each plane file, one with _denoised
// appended to its stem. In shared mode the first set also writes the filtered sum of its planes to
// <out>_denoised.exr, unless --denoise is given, whose file that is. The planes' own files are the same
// bytes with or without it. Without a plane flag, with another value or with an empty --sample-window it
// is refused before any device is used.
// --batches K (2..64, any of the three integrators; one device, no plane flag) renders the frame as K
// batches, the windows (first + b stride, stride K, count / K) of --sample-window's window or of the whole
// spp, whose count must be a multiple of K. The main EXR is bdpt_batch_moments_host's sum of them (the plain
// frame up to the order of the float additions), and <out>_variance.exr the per-pixel variance of that
// sum, three channels. --denoise-var[=ITER] (with --batches; not with --denoise, whose file it writes) also
// renders the feature buffers over the same samples and writes <out>_denoised.exr from
// bdpt_denoise_var_host (the header's BDPT_DENOISE_VAR_* defaults, ITER iterations 0..8). Combines with
// --aov. Each misuse is refused, the flag named, before any device is used.
// --adaptive THR[:K[:STEP[:PASSES]]] (a bdpt scene, one device) renders with bdpt_render_adaptive_host: spp is
// the budget per pixel and must equal PASSES * STEP * K (K batches, default 8; STEP samples per batch and
// pass, default 1; PASSES default spp / (STEP * K)); a pixel gets further passes while its relative standard
// deviation across the batches exceeds THR. Writes the frame, <out>_variance.exr (its per-pixel variance)
// and <out>_samples.exr (the samples each pixel had, as a grey value). Refused, the flag named, with --gpus /
// --devices, --layers, --light-groups, --strategies, --batches, --cross, --denoise-planes and --sample-window.
// --cameras FILE --temporal[=MAXHIST] (a bdpt scene, one device) renders a camera sequence with temporal accumulation
// (bdpt_reproject_host, the header's BDPT_REPROJECT_* defaults, MAXHIST > 0 in place of its history cap). FILE has one
// line per frame, ex ey ez ax ay az ux uy uz fov (eye, at, up, fov in degrees); blank lines and lines starting
// with # are skipped. Frame f is rendered at the TOML's spp from camera f, its seed base moved on by f * width *
// height * spp so that no two frames repeat a sample, and blended with the history of frame f - 1: <out
// stem>.f<nn>.exr is the accumulated frame (frame 0: the plain render of camera 0), and with --denoise <out
// stem>.f<nn>_denoised.exr the filter of the accumulated frame under that frame's feature buffers, norm 1. The TOML's
// own camera is not rendered and <out> itself is not written. Refused, the flag named, before any device is
// used: one flag without the other, an unreadable or malformed FILE, a path / direct scene, and --gpus /
// --devices, --layers, --light-groups, --strategies, --cross, --denoise-planes, --batches, --denoise-var,
// --adaptive, --sample-window and --aov.
// --display[=png|ppm] (default png) also writes an 8-bit image beside the EXRs, the same name with the extension
// .png / .ppm: <out stem>.png from the last colour the command made (the plain frame, or <out>_denoised.exr's with
// --denoise / --denoise-var; --adaptive's frame), through bdpt_meter_host and bdpt_display_host. --exposure
// auto[:KEY[:RATE]] (the default; the header's BDPT_METER_* otherwise) meters the frame, under the feature buffers
// when the command rendered them; --exposure EV shows it at 2^EV. --tone clamp|reinhard|filmic (default reinhard),
// --encode srgb|gamma22|linear (default srgb). With --cameras --temporal every frame gets <out stem>.f<nn>.png, its
// exposure adapted from the frame before at RATE. The planes of --layers, --light-groups, --strategies and --cross
// get one file each, all shown with the sum frame's meter words, so that they stay comparable. The EXRs are the
// same bytes with or without it; with several devices the first one displays. A bad value of any of the four
// flags, or one of the last three without --display, is refused, the flag named, before any device is used.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bdpt_amd.h"

namespace {

int die(const char* what) {
    std::fprintf(stderr, "%s: %s\n", what, bdpt_last_error());
    return EXIT_FAILURE;
}

// fs::path::replace_extension("exr") on the TOML path (integrator.cpp:28).
std::string exr_path_of(const std::string& toml) {
    const size_t slash = toml.find_last_of('/');
    const size_t dot = toml.find_last_of('.');
    const size_t name = slash == std::string::npos ? 0 : slash + 1;
    // a leading dot names the file (".toml"), it is not an extension
    if (dot == std::string::npos || dot <= name || (dot == name && toml.size() > name)) return toml + ".exr";
    return toml.substr(0, dot) + ".exr";
}

// "F:S:C", three integers and nothing else.
bool parse_window(const char* text, bdpt_sample_window* w) {
    int32_t* const field[3] = {&w->first, &w->stride, &w->count};
    const char* q = text;
    for (int k = 0; k < 3; k++) {
        char* end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q || v < INT32_MIN || v > INT32_MAX) return false;
        if (*end != (k < 2 ? ':' : '\0')) return false;
        *field[k] = static_cast<int32_t>(v);
        q = end + 1;
    }
    return true;
}

// "<out minus .exr><suffix>.exr"
std::string side_path(const std::string& exr, const char* suffix) {
    const bool ext = exr.size() >= 4 && exr.compare(exr.size() - 4, 4, ".exr") == 0;
    return (ext ? exr.substr(0, exr.size() - 4) : exr) + suffix + ".exr";
}

// --cameras FILE: ten numbers per line (eye, at, up, fov); blank lines and # lines skipped. false with a message.
bool parse_cameras(const std::string& file, std::vector<bdpt_camera>* out, std::string* error) {
    std::ifstream in(file);
    if (!in) {
        *error = "cannot read the file";
        return false;
    }
    std::string line;
    for (int n = 1; std::getline(in, line); n++) {
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        std::istringstream fields(line);
        float v[10];
        int got = 0;
        while (got < 10 && fields >> v[got]) got++;
        std::string rest;
        if (got < 10 || (fields >> rest)) {  // too few, not a number, or something after the tenth
            *error = "line " + std::to_string(n) + ": expected ten numbers (ex ey ez ax ay az ux uy uz fov)";
            return false;
        }
        bdpt_camera c;
        for (int k = 0; k < 3; k++) c.eye[k] = v[k], c.at[k] = v[3 + k], c.up[k] = v[6 + k];
        c.fov = v[9];
        if (!(c.fov > 0.f && c.fov < 180.f)) {
            *error = "line " + std::to_string(n) + ": fov must be in (0, 180) degrees";
            return false;
        }
        out->push_back(c);
    }
    if (out->empty()) {
        *error = "no camera line";
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "Syntax: %s <scene.toml> [nogui] [--width W --height H --spp N --rr D --device K "
                             "--out FILE.exr --seed S --gpus N --devices a,b,... --shard samples|rows "
                             "--sample-window F:S:C --aov --denoise[=ITER] --layers N --light-groups --strategies[=unweighted] --cross --denoise-planes[=own|shared] --batches K --denoise-var[=ITER] --adaptive THR[:K[:STEP[:PASSES]]] --cameras FILE --temporal[=MAXHIST] --display[=png|ppm] --exposure auto[:KEY[:RATE]]|EV --tone clamp|reinhard|filmic --encode srgb|gamma22|linear]\n", argv[0]);
        return EXIT_FAILURE;
    }
    const std::string toml = argv[1];
    int W = -1, H = -1, spp = -1, rr = -1, device = 0;
    long long seed = -1;
    std::string out;
    std::vector<int32_t> devices;  // non-empty: the multi-device render
    int32_t sharding = BDPT_SHARD_ROWS;
    bool shard_given = false, windowed = false;
    bdpt_sample_window window = {0, 1, 0};
    bool want_aov = false, want_denoise = false;
    int denoise_iterations = BDPT_DENOISE_ITERATIONS;
    int layers = 0;  // --layers N (0: none)
    bool light_groups = false;  // --light-groups
    int strategies = -1;        // --strategies[=unweighted]: BDPT_STRATEGIES_* (-1: none)
    bool cross = false;         // --cross: the groups crossed with the layers or the strategies
    int denoise_planes = -1;    // --denoise-planes[=own|shared]: BDPT_DENOISE_PLANES_* (-1: none)
    int batches = 0;            // --batches K (0: none)
    bool adaptive = false;      // --adaptive THR[:K[:STEP[:PASSES]]]
    bdpt_adaptive_params ad = {8, 1, 0, 0.f, 1e-3f, 1, 0};  // (max_passes 0: spp / (step * n_batches))
    bool want_denoise_var = false;  // --denoise-var[=ITER]
    int denoise_var_iterations = BDPT_DENOISE_VAR_ITERATIONS;
    bool temporal = false;          // --temporal[=MAXHIST]
    float temporal_max_history = BDPT_REPROJECT_MAX_HISTORY;
    std::string cameras_file;       // --cameras FILE
    std::vector<bdpt_camera> cameras;
    enum { DISPLAY_NONE, DISPLAY_PNG, DISPLAY_PPM } display = DISPLAY_NONE;  // --display[=png|ppm]
    bool exposure_auto = true, exposure_given = false, tone_given = false, encode_given = false;
    bdpt_meter_params meter = {1.f, BDPT_METER_KEY, BDPT_METER_KEY_PERMILLE, BDPT_METER_WHITE_PERMILLE, BDPT_METER_RATE, 1.f, 1.f};
    bdpt_display_params shown = {1.f, 1.f, 1.f, BDPT_TONE_REINHARD, BDPT_ENCODE_SRGB, 3};
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&](const char* flag) -> const char* {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "%s needs a value\n", flag);
                std::exit(EXIT_FAILURE);
            }
            return argv[++i];
        };
        if (a == "nogui") continue;  // there is no GUI on this path
        else if (a == "--width") W = std::atoi(next("--width"));
        else if (a == "--height") H = std::atoi(next("--height"));
        else if (a == "--spp") spp = std::atoi(next("--spp"));
        else if (a == "--rr") rr = std::atoi(next("--rr"));
        else if (a == "--device") device = std::atoi(next("--device"));
        else if (a == "--seed") seed = std::atoll(next("--seed"));
        else if (a == "--out") out = next("--out");
        else if (a == "--shard") {
            const std::string v = next("--shard");
            if (v != "samples" && v != "rows") {
                std::fprintf(stderr, "--shard must be samples or rows, not %s\n", v.c_str());
                return EXIT_FAILURE;
            }
            sharding = v == "samples" ? BDPT_SHARD_SAMPLES : BDPT_SHARD_ROWS;
            shard_given = true;
        } else if (a == "--sample-window") {
            const char* v = next("--sample-window");
            if (!parse_window(v, &window)) {
                std::fprintf(stderr, "--sample-window %s: expected first:stride:count (three integers)\n", v);
                return EXIT_FAILURE;
            }
            if (window.first < 0 || window.stride < 1 || window.count < 0) {
                std::fprintf(stderr, "--sample-window %s: %s\n", v,
                             window.first < 0 ? "first must be >= 0"
                                              : window.stride < 1 ? "stride must be >= 1" : "count must be >= 0");
                return EXIT_FAILURE;
            }
            windowed = true;
        } else if (a == "--aov") {
            want_aov = true;
        } else if (a == "--denoise") {
            want_denoise = true;
        } else if (a.compare(0, 10, "--denoise=") == 0) {
            const char* v = argv[i] + 10;
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 0 || n > 8) {
                std::fprintf(stderr, "--denoise=%s: the iteration count must be an integer in [0, 8]\n", v);
                return EXIT_FAILURE;
            }
            want_denoise = true;
            denoise_iterations = static_cast<int>(n);
        } else if (a == "--denoise-var") {
            want_denoise_var = true;
        } else if (a.compare(0, 14, "--denoise-var=") == 0) {
            const char* v = argv[i] + 14;
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 0 || n > 8) {
                std::fprintf(stderr, "--denoise-var=%s: the iteration count must be an integer in [0, 8]\n", v);
                return EXIT_FAILURE;
            }
            want_denoise_var = true;
            denoise_var_iterations = static_cast<int>(n);
        } else if (a.rfind("--denoise-var", 0) == 0) {
            std::fprintf(stderr, "%s: --denoise-var takes no value or =ITER\n", a.c_str());
            return EXIT_FAILURE;
        } else if (a == "--batches") {
            const char* v = next("--batches");
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 2 || n > 64) {
                std::fprintf(stderr, "--batches %s: the batch count must be an integer in [2, 64]\n", v);
                return EXIT_FAILURE;
            }
            batches = static_cast<int>(n);
        } else if (a == "--adaptive") {
            const char* v = next("--adaptive");
            char* end = nullptr;
            ad.threshold = std::strtof(v, &end);
            long f[3] = {ad.n_batches, ad.step, 0};
            bool ok = end != v && ad.threshold >= 0.f && ad.threshold < 1e30f;
            for (int k = 0; ok && k < 3 && *end == ':'; k++) {
                const char* q = end + 1;
                f[k] = std::strtol(q, &end, 10);
                ok = end != q && f[k] >= 1 && f[k] <= 1 << 20;
            }
            if (!ok || *end != '\0' || f[0] < 2 || f[0] > 64 || f[2] > BDPT_ADAPTIVE_MAX_PASSES) {
                std::fprintf(stderr, "--adaptive %s: THR[:K[:STEP[:PASSES]]] with THR >= 0, K in [2, 64], STEP >= 1, PASSES in [1, %d]\n",
                             v, BDPT_ADAPTIVE_MAX_PASSES);
                return EXIT_FAILURE;
            }
            adaptive = true;
            ad.n_batches = static_cast<int32_t>(f[0]), ad.step = static_cast<int32_t>(f[1]), ad.max_passes = static_cast<int32_t>(f[2]);
        } else if (a == "--cameras") {
            cameras_file = next("--cameras");
        } else if (a == "--temporal") {
            temporal = true;
        } else if (a.compare(0, 11, "--temporal=") == 0) {
            const char* v = argv[i] + 11;
            char* end = nullptr;
            temporal_max_history = std::strtof(v, &end);
            if (end == v || *end != '\0' || !(temporal_max_history > 0.f) || !(temporal_max_history < 1e30f)) {
                std::fprintf(stderr, "--temporal=%s: the history cap must be a number > 0\n", v);
                return EXIT_FAILURE;
            }
            temporal = true;
        } else if (a.rfind("--temporal", 0) == 0) {
            std::fprintf(stderr, "%s: --temporal takes no value or =MAXHIST\n", a.c_str());
            return EXIT_FAILURE;
        } else if (a == "--display" || a == "--display=png") {
            display = DISPLAY_PNG;
        } else if (a == "--display=ppm") {
            display = DISPLAY_PPM;
        } else if (a.rfind("--display", 0) == 0) {
            std::fprintf(stderr, "%s: --display takes no value, =png or =ppm\n", a.c_str());
            return EXIT_FAILURE;
        } else if (a == "--exposure") {
            const std::string v = next("--exposure");
            bool ok = true;
            if (v.compare(0, 4, "auto") == 0) {  // auto[:KEY[:RATE]]
                exposure_auto = true;
                const char* q = v.c_str() + 4;
                float* const field[2] = {&meter.key, &meter.rate};
                for (int k = 0; ok && k < 2 && *q == ':'; k++) {
                    char* end = nullptr;
                    *field[k] = std::strtof(q + 1, &end);
                    ok = end != q + 1;
                    q = end;
                }
                ok = ok && *q == '\0' && meter.key > 0.f && meter.key < 1e30f && meter.rate > 0.f && meter.rate <= 1.f;
            } else {  // EV, in stops
                char* end = nullptr;
                const double ev = std::strtod(v.c_str(), &end);
                ok = end != v.c_str() && *end == '\0' && ev >= -64. && ev <= 64.;
                if (ok) exposure_auto = false, shown.exposure = static_cast<float>(std::exp2(ev));
            }
            if (!ok) {
                std::fprintf(stderr, "--exposure %s: auto[:KEY[:RATE]] with KEY > 0 and RATE in (0, 1], or EV, a number of stops in [-64, 64]\n",
                             v.c_str());
                return EXIT_FAILURE;
            }
            exposure_given = true;
        } else if (a == "--tone") {
            const std::string v = next("--tone");
            if (v != "clamp" && v != "reinhard" && v != "filmic") {
                std::fprintf(stderr, "--tone must be clamp, reinhard or filmic, not %s\n", v.c_str());
                return EXIT_FAILURE;
            }
            shown.tone = v == "clamp" ? BDPT_TONE_CLAMP : v == "reinhard" ? BDPT_TONE_REINHARD : BDPT_TONE_FILMIC;
            tone_given = true;
        } else if (a == "--encode") {
            const std::string v = next("--encode");
            if (v != "srgb" && v != "gamma22" && v != "linear") {
                std::fprintf(stderr, "--encode must be srgb, gamma22 or linear, not %s\n", v.c_str());
                return EXIT_FAILURE;
            }
            shown.encode = v == "srgb" ? BDPT_ENCODE_SRGB : v == "gamma22" ? BDPT_ENCODE_GAMMA22 : BDPT_ENCODE_LINEAR;
            encode_given = true;
        } else if (a == "--denoise-planes" || a == "--denoise-planes=shared") {
            denoise_planes = BDPT_DENOISE_PLANES_SHARED;
        } else if (a == "--denoise-planes=own") {
            denoise_planes = BDPT_DENOISE_PLANES_OWN;
        } else if (a.rfind("--denoise-planes", 0) == 0) {
            std::fprintf(stderr, "%s: --denoise-planes takes no value, =own or =shared\n", a.c_str());
            return EXIT_FAILURE;
        } else if (a == "--layers") {
            const char* v = next("--layers");
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 64) {
                std::fprintf(stderr, "--layers %s: the layer count must be an integer in [1, 64]\n", v);
                return EXIT_FAILURE;
            }
            layers = static_cast<int>(n);
        } else if (a == "--light-groups") {
            light_groups = true;
        } else if (a == "--cross") {
            cross = true;
        } else if (a == "--strategies" || a == "--strategies=weighted") {
            strategies = BDPT_STRATEGIES_WEIGHTED;
        } else if (a == "--strategies=unweighted") {
            strategies = BDPT_STRATEGIES_UNWEIGHTED;
        } else if (a.rfind("--strategies", 0) == 0) {
            std::fprintf(stderr, "%s: --strategies takes no value, =weighted or =unweighted\n", a.c_str());
            return EXIT_FAILURE;
        } else if (a == "--gpus") {
            const int n = std::atoi(next("--gpus"));
            devices.clear();
            for (int k = 0; k < n; k++) devices.push_back(k);
        } else if (a == "--devices") {
            devices.clear();
            for (const char* q = next("--devices"); *q;) {
                devices.push_back(static_cast<int32_t>(std::strtol(q, const_cast<char**>(&q), 10)));
                if (*q == ',') q++;
                else if (*q) break;
            }
        }
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return EXIT_FAILURE;
        }
    }
    if (windowed && !devices.empty()) {
        std::fprintf(stderr, "--sample-window renders on one device (--gpus / --devices split the frame themselves)\n");
        return EXIT_FAILURE;
    }
    if (display != DISPLAY_NONE && windowed && window.count == 0) {
        std::fprintf(stderr, "--display of an empty --sample-window (count 0): there is no sample to normalise by\n");
        return EXIT_FAILURE;
    }
    if (want_denoise && windowed && window.count == 0) {
        std::fprintf(stderr, "--denoise of an empty --sample-window (count 0): there is no sample to normalise by\n");
        return EXIT_FAILURE;
    }
    if (denoise_planes >= 0 && !layers && !light_groups && strategies < 0) {
        std::fprintf(stderr, "--denoise-planes filters the planes of --layers N, --light-groups or --strategies: give one of them\n");
        return EXIT_FAILURE;
    }
    if (denoise_planes >= 0 && windowed && window.count == 0) {
        std::fprintf(stderr, "--denoise-planes of an empty --sample-window (count 0): there is no sample to normalise by\n");
        return EXIT_FAILURE;
    }
    if (want_denoise_var && !batches) {
        std::fprintf(stderr, "--denoise-var filters with the variance across batches: give --batches K\n");
        return EXIT_FAILURE;
    }
    if (want_denoise_var && want_denoise) {
        std::fprintf(stderr, "--denoise-var and --denoise both write <out>_denoised.exr: give one of them\n");
        return EXIT_FAILURE;
    }
    if (batches && !devices.empty()) {
        std::fprintf(stderr, "--batches renders on one device (not with --gpus / --devices)\n");
        return EXIT_FAILURE;
    }
    if (batches && (layers || light_groups || strategies >= 0 || cross || denoise_planes >= 0)) {
        std::fprintf(stderr, "--batches splits the frame by samples: not with --layers, --light-groups, --strategies, "
                             "--cross or --denoise-planes\n");
        return EXIT_FAILURE;
    }
    if (adaptive) {
        const char* with = !devices.empty() ? "--gpus / --devices" : layers ? "--layers" : light_groups ? "--light-groups"
                           : strategies >= 0 ? "--strategies" : batches ? "--batches" : cross ? "--cross"
                           : denoise_planes >= 0 ? "--denoise-planes" : windowed ? "--sample-window" : nullptr;
        if (with) {
            std::fprintf(stderr, "--adaptive chooses each pixel's samples itself, on one device and one frame: not with %s\n", with);
            return EXIT_FAILURE;
        }
    }
    if (temporal != !cameras_file.empty()) {
        std::fprintf(stderr, temporal ? "--temporal accumulates over a camera sequence: give --cameras FILE\n"
                                      : "--cameras is the sequence --temporal[=MAXHIST] renders: give that flag\n");
        return EXIT_FAILURE;
    }
    if (temporal) {
        const char* with = !devices.empty() ? "--gpus / --devices" : layers ? "--layers" : light_groups ? "--light-groups"
                           : strategies >= 0 ? "--strategies" : cross ? "--cross" : denoise_planes >= 0 ? "--denoise-planes"
                           : batches ? "--batches" : want_denoise_var ? "--denoise-var" : adaptive ? "--adaptive"
                           : windowed ? "--sample-window" : want_aov ? "--aov" : nullptr;
        if (with) {
            std::fprintf(stderr, "--temporal renders whole frames of a camera sequence on one device: not with %s\n", with);
            return EXIT_FAILURE;
        }
        std::string error;
        if (!parse_cameras(cameras_file, &cameras, &error)) {
            std::fprintf(stderr, "--cameras %s: %s\n", cameras_file.c_str(), error.c_str());
            return EXIT_FAILURE;
        }
    }
    if (display == DISPLAY_NONE && (exposure_given || tone_given || encode_given)) {
        std::fprintf(stderr, "%s sets how --display[=png|ppm] shows the frame: give that flag\n",
                     exposure_given ? "--exposure" : tone_given ? "--tone" : "--encode");
        return EXIT_FAILURE;
    }
    if (shard_given && devices.empty()) {
        std::fprintf(stderr, "--shard applies to a multi-device render (--gpus N / --devices a,b,...)\n");
        return EXIT_FAILURE;
    }

    bdpt_config cfg;
    if (bdpt_config_load_toml(toml.c_str(), &cfg) != BDPT_OK) {
        std::fprintf(stderr, "Error while parsing scene file: %s\n", bdpt_last_error());  // main.cpp:128-131
        return EXIT_FAILURE;
    }
    if (cfg.realtime) {
        std::fprintf(stderr, "realtime render passes are not part of the MI355X BDPT path\n");
        return EXIT_FAILURE;
    }
    std::printf("%s\n", cfg.integrator);  // main.cpp:72
    const bool path = std::strcmp(cfg.integrator, "path") == 0;
    const bool direct = std::strcmp(cfg.integrator, "direct") == 0;
    if (!path && !direct && std::strcmp(cfg.integrator, "bdpt") != 0) {
        std::fprintf(stderr, "integrator type \"%s\" is not part of the MI355X BDPT path\n", cfg.integrator);
        return EXIT_FAILURE;
    }
    if (cross && (!light_groups || (layers != 0) == (strategies >= 0))) {
        std::fprintf(stderr, "--cross takes --light-groups and exactly one of --layers N / --strategies[=unweighted]\n");
        return EXIT_FAILURE;
    }
    if (layers && (path || direct)) {
        std::fprintf(stderr, "--layers splits a bdpt frame (integrator type \"%s\" has no layers)\n", cfg.integrator);
        return EXIT_FAILURE;
    }
    if (light_groups && (path || direct)) {
        std::fprintf(stderr, "--light-groups splits a bdpt frame (integrator type \"%s\" has no light groups)\n",
                     cfg.integrator);
        return EXIT_FAILURE;
    }
    if (strategies >= 0 && (path || direct)) {
        std::fprintf(stderr, "--strategies splits a bdpt frame (integrator type \"%s\" has no (s, t) strategies)\n",
                     cfg.integrator);
        return EXIT_FAILURE;
    }
    if (temporal && (path || direct)) {
        std::fprintf(stderr, "--temporal accumulates a bdpt frame sequence (integrator type \"%s\" has no sequence loop)\n",
                     cfg.integrator);
        return EXIT_FAILURE;
    }
    if (adaptive && (path || direct)) {
        std::fprintf(stderr, "--adaptive samples a bdpt frame (integrator type \"%s\" has no pixel-list kernel)\n", cfg.integrator);
        return EXIT_FAILURE;
    }
    if (W > 0) cfg.width = W;
    if (H > 0) cfg.height = H;
    if (spp > 0) cfg.spp = spp;
    if (rr > 0) cfg.rr_depth = rr;
    if (adaptive) {  // spp is the budget: PASSES * STEP * K
        const int per_pass = ad.step * ad.n_batches;
        if (ad.max_passes == 0) ad.max_passes = cfg.spp / per_pass;
        if (ad.max_passes < 1 || ad.max_passes > BDPT_ADAPTIVE_MAX_PASSES ||
            static_cast<long long>(ad.max_passes) * per_pass != cfg.spp) {
            std::fprintf(stderr, "--adaptive: spp (%d) must be PASSES * STEP * K with PASSES in [1, %d] (STEP * K = %d)\n",
                         cfg.spp, BDPT_ADAPTIVE_MAX_PASSES, per_pass);
            return EXIT_FAILURE;
        }
    }
    int32_t n_s = 0, n_t = 0;  // --strategies: the shape that clamps nothing
    if (strategies >= 0 && bdpt_strategies_shape(cfg.rr_depth, BDPT_STRATEGY_BDPT, &n_s, &n_t) != BDPT_OK)
        return die("--strategies");
    if (windowed && window.count > 0 &&
        static_cast<long long>(window.first) + static_cast<long long>(window.count - 1) * window.stride >= cfg.spp) {
        std::fprintf(stderr, "--sample-window %d:%d:%d: count reaches past spp = %d\n", window.first, window.stride,
                     window.count, cfg.spp);
        return EXIT_FAILURE;
    }

    if (batches) {  // equal batches: what the variance formula assumes
        const int count = windowed ? window.count : cfg.spp;
        if (count < 1 || count % batches != 0) {
            std::fprintf(stderr, "--batches %d: the %s (%d) must be a positive multiple of the batch count\n", batches,
                         windowed ? "--sample-window count" : "spp", count);
            return EXIT_FAILURE;
        }
    }

    bdpt_scene* scene = nullptr;
    if (bdpt_scene_load_obj(cfg.obj_file, &scene) != BDPT_OK) return die("Scene::load");
    int32_t n_emitters = 0;
    if (light_groups) {  // one plane per emitter: refused before any device is used
        if (bdpt_scene_emitter_count(scene, &n_emitters) != BDPT_OK) return die("bdpt_scene_emitter_count");
        if (n_emitters > 64) {
            std::fprintf(stderr, "--light-groups: the scene has %d emitters, one plane each is built for at most 64\n",
                         n_emitters);
            return EXIT_FAILURE;
        }
    }
    bdpt_ctx* ctx = nullptr;
    bdpt_multi* multi = nullptr;
    if (!devices.empty()) {
        if (bdpt_multi_create(scene, static_cast<int32_t>(devices.size()), devices.data(), &multi) != BDPT_OK)
            return die("bdpt_multi_create");
        if (bdpt_multi_set_sharding(multi, sharding) != BDPT_OK) return die("bdpt_multi_set_sharding");
    } else if (bdpt_ctx_create(scene, device, &ctx) != BDPT_OK) {
        return die("bdpt_ctx_create");
    }

    bdpt_frame_params p;
    std::memset(&p, 0, sizeof(p));
    p.camera = cfg.camera;
    p.width = cfg.width;
    p.height = cfg.height;
    p.spp = cfg.spp;
    p.rr_depth = cfg.rr_depth;
    p.strategy = BDPT_STRATEGY_BDPT;
    p.seed_base = seed >= 0 ? static_cast<uint32_t>(seed) : 260450963u;  // renderer.cpp:155
    p.row_offset = 0;
    p.row_stride = 1;
    std::vector<float> rgb(static_cast<size_t>(cfg.width) * cfg.height * 3, 0.f);  // Integrator::init: rgb->clear()

    // --display: the 8-bit image of `color` beside the EXR `exr_name`, its extension .png / .ppm. With --exposure
    // auto the exposure and white point come from meter words: measure = true meters color (under aov, NULL:
    // every pixel; adapted from prev, NULL: none) into words first, measure = false shows it with the words given.
    auto write_display = [&](bdpt_ctx* dctx, const float* color, const float* aov, const uint32_t* prev, uint32_t* words,
                             bool measure, float norm, const std::string& exr_name) -> int {
        if (exposure_auto && measure) {
            bdpt_meter_params m = meter;
            m.norm = norm;
            if (bdpt_meter_host(dctx, cfg.width, cfg.height, color, aov, prev, &m, words) != BDPT_OK) return die("bdpt_meter_host");
        }
        bdpt_display_params d = shown;
        d.norm = norm;
        std::vector<unsigned char> bytes(static_cast<size_t>(cfg.width) * cfg.height * 3);
        if (bdpt_display_host(dctx, cfg.width, cfg.height, color, exposure_auto ? words : nullptr, &d, bytes.data()) != BDPT_OK)
            return die("bdpt_display_host");
        const std::string stem = side_path(exr_name, "");
        const std::string file = stem.substr(0, stem.size() - 4) + (display == DISPLAY_PNG ? ".png" : ".ppm");
        const int rc = display == DISPLAY_PNG ? bdpt_save_png(bytes.data(), cfg.width, cfg.height, 3, file.c_str())
                                              : bdpt_save_ppm(bytes.data(), cfg.width, cfg.height, file.c_str());
        if (rc != BDPT_OK) return die(display == DISPLAY_PNG ? "bdpt_save_png" : "bdpt_save_ppm");
        std::printf("Saved %s image to %s\n", display == DISPLAY_PNG ? "PNG" : "PPM", file.c_str());
        return EXIT_SUCCESS;
    };

    if (temporal) {  // the camera sequence: render, feature buffers, reproject, per frame
        uint32_t words[2][4] = {};  // --display: the meter words of this frame and of the one before
        const std::string exr = out.empty() ? exr_path_of(toml) : out;
        const size_t px = static_cast<size_t>(cfg.width) * cfg.height;
        std::vector<float> aov(px * 8), acc(px * 3), den(px * 3), hist[2] = {std::vector<float>(px * 8), std::vector<float>(px * 8)};
        const uint32_t seed0 = p.seed_base;
        const auto t0 = std::chrono::high_resolution_clock::now();
        for (size_t f = 0; f < cameras.size(); f++) {
            p.camera = cameras[f];
            p.seed_base = seed0 + static_cast<uint32_t>(f * px * static_cast<size_t>(cfg.spp));
            std::fill(rgb.begin(), rgb.end(), 0.f);
            std::fill(aov.begin(), aov.end(), 0.f);
            if (bdpt_render_window_host(ctx, &p, nullptr, nullptr, nullptr, rgb.data()) != BDPT_OK) return die("render (bdpt)");
            if (bdpt_render_aov_host(ctx, &p, nullptr, aov.data()) != BDPT_OK) return die("bdpt_render_aov_host");
            const bdpt_reproject_params r = {cameras[f ? f - 1 : 0], 1.f, static_cast<float>(cfg.spp), temporal_max_history,
                                             BDPT_REPROJECT_SIGMA_NORMAL, BDPT_REPROJECT_SIGMA_DEPTH, BDPT_REPROJECT_MIN_WEIGHT,
                                             BDPT_REPROJECT_CLAMP_SIGMA, BDPT_REPROJECT_DEMODULATE};
            if (bdpt_reproject_host(ctx, &p, rgb.data(), aov.data(), f ? hist[(f - 1) & 1].data() : nullptr, acc.data(),
                                    hist[f & 1].data(), &r) != BDPT_OK)
                return die("bdpt_reproject_host");
            char suffix[32];
            std::snprintf(suffix, sizeof suffix, ".f%02d", static_cast<int>(f));
            const std::string frame = side_path(exr, suffix);
            if (bdpt_save_exr(acc.data(), cfg.width, cfg.height, frame.c_str()) != BDPT_OK) return die("saveEXR");
            std::printf("Saved EXR image to %s\n", frame.c_str());
            if (want_denoise) {
                const bdpt_denoise_params d = {denoise_iterations, BDPT_DENOISE_SIGMA_COLOR, BDPT_DENOISE_SIGMA_NORMAL,
                                               BDPT_DENOISE_SIGMA_DEPTH, BDPT_DENOISE_DEMODULATE, 1.f};
                if (bdpt_denoise_host(ctx, cfg.width, cfg.height, acc.data(), aov.data(), den.data(), &d) != BDPT_OK)
                    return die("bdpt_denoise_host");
                const std::string side = side_path(exr, (std::string(suffix) + "_denoised").c_str());
                if (bdpt_save_exr(den.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
                std::printf("Saved EXR image to %s\n", side.c_str());
            }
            if (display != DISPLAY_NONE) {  // the frame's last colour, its exposure adapted from the frame before
                if (const int rc = write_display(ctx, want_denoise ? den.data() : acc.data(), aov.data(), f ? words[(f - 1) & 1] : nullptr,
                                                 words[f & 1], true, 1.f, frame))
                    return rc;
            }
        }
        const auto t1 = std::chrono::high_resolution_clock::now();
        std::printf("Render took: %g seconds.\n", std::chrono::duration<double>(t1 - t0).count());
        bdpt_ctx_destroy(ctx);
        bdpt_scene_free(scene);
        return EXIT_SUCCESS;
    }

    const bdpt_sample_window* const win = windowed ? &window : nullptr;  // null: every sample
    // --batches: the K planes (plane b: the window's samples b, b + K, ...), then their sum in rgb and its variance
    std::vector<float> batch_planes, variance;
    std::vector<int32_t> sample_map;  // --adaptive: samples per pixel
    bdpt_adaptive_stats ad_stats{};
    auto render_window = [&](const bdpt_path_params* pp, const bdpt_direct_params* dp) -> int {
        if (adaptive) {
            variance.resize(rgb.size());
            sample_map.resize(rgb.size() / 3);
            return bdpt_render_adaptive_host(ctx, &p, &ad, rgb.data(), variance.data(), sample_map.data(), &ad_stats);
        }
        if (!batches) return bdpt_render_window_host(ctx, &p, win, pp, dp, rgb.data());
        const bdpt_sample_window base = windowed ? window : bdpt_sample_window{0, 1, cfg.spp};
        batch_planes.assign(rgb.size() * batches, 0.f);
        for (int b = 0; b < batches; b++) {
            const bdpt_sample_window w = {base.first + b * base.stride, base.stride * batches, base.count / batches};
            if (const int rc = bdpt_render_window_host(ctx, &p, &w, pp, dp, batch_planes.data() + rgb.size() * b)) return rc;
        }
        variance.resize(rgb.size());
        return bdpt_batch_moments_host(ctx, cfg.width, cfg.height, batches, batch_planes.data(), rgb.data(), variance.data());
    };
    const auto t0 = std::chrono::high_resolution_clock::now();
    if (path) {
        if (rr > 0) cfg.path.rr_depth = rr;
        p.rr_depth = 1;  // unused by the path tracer
        const int rc = multi ? bdpt_multi_render_host(multi, &p, &cfg.path, nullptr, rgb.data())
                             : render_window(&cfg.path, nullptr);
        if (rc != BDPT_OK) return die("render (path)");
    } else if (direct) {
        p.rr_depth = 1;  // unused by the direct integrator
        const int rc = multi ? bdpt_multi_render_host(multi, &p, nullptr, &cfg.direct, rgb.data())
                             : render_window(nullptr, &cfg.direct);
        if (rc != BDPT_OK) {
            if (cfg.direct.sampling_strategy == 0) {  // direct.h:460-461
                std::printf("Error: wrong strategy\n");
                return EXIT_FAILURE;
            }
            return die("render (direct)");
        }
    } else if ((multi ? bdpt_multi_render_host(multi, &p, nullptr, nullptr, rgb.data())
                      : render_window(nullptr, nullptr)) != BDPT_OK) {
        return die("render (bdpt)");
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    std::printf("Render took: %g seconds.\n", std::chrono::duration<double>(t1 - t0).count());
    if (multi) {
        bdpt_multi_stats st;
        bdpt_multi_get_stats(multi, &st);
        std::printf("%d devices (%s): render %.3f ms, reduce %.3f ms\n", st.devices, st.rccl ? "RCCL reduce" : "local sum",
                    st.render_ms, st.reduce_ms);
    }

    const std::string exr = out.empty() ? exr_path_of(toml) : out;
    if (bdpt_save_exr(rgb.data(), cfg.width, cfg.height, exr.c_str()) != BDPT_OK) return die("saveEXR");
    std::printf("\nSaved EXR image to %s\n", exr.c_str());  // utils.h:149
    if (adaptive) {
        std::printf("adaptive: %d passes, %lld samples (uniform: %lld)\n", ad_stats.passes,
                    static_cast<long long>(ad_stats.samples), static_cast<long long>(sample_map.size()) * cfg.spp);
        std::vector<float> grey(rgb.size());
        for (size_t i = 0; i < sample_map.size(); i++) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = static_cast<float>(sample_map[i]);
        const std::string side = side_path(exr, "_samples");
        if (bdpt_save_exr(grey.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
        std::printf("Saved EXR image to %s\n", side.c_str());
    }
    if (batches || adaptive) {
        const std::string side = side_path(exr, "_variance");
        if (bdpt_save_exr(variance.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
        std::printf("Saved EXR image to %s\n", side.c_str());
    }
    // --display shows the last colour the command made (the filtered frame if there is one) and meters it under
    // the feature buffers when the command rendered them
    std::vector<float> shown_color, shown_aov;
    if (want_aov || want_denoise || want_denoise_var) {
        bdpt_ctx* fctx = ctx;  // several devices: the first renders the feature buffers and filters
        if (!fctx && bdpt_ctx_create(scene, devices[0], &fctx) != BDPT_OK) return die("bdpt_ctx_create (feature buffers)");
        const size_t px = static_cast<size_t>(cfg.width) * cfg.height;
        std::vector<float> aov(px * 8, 0.f);
        if (bdpt_render_aov_host(fctx, &p, win, aov.data()) != BDPT_OK) return die("bdpt_render_aov_host");
        if (want_aov) {
            std::vector<float> img(px * 3);
            for (int part = 0; part < 2; part++) {  // albedo, normal: divided by the coverage, 0 where nothing was hit
                for (size_t i = 0; i < px; i++)
                    for (int ch = 0; ch < 3; ch++)
                        img[3 * i + ch] = aov[8 * i + 7] > 0.f ? aov[8 * i + 3 * part + ch] / aov[8 * i + 7] : 0.f;
                const std::string side = side_path(exr, part ? "_normal" : "_albedo");
                if (bdpt_save_exr(img.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
                std::printf("Saved EXR image to %s\n", side.c_str());
            }
        }
        if (want_denoise) {
            bdpt_denoise_params d = {denoise_iterations, BDPT_DENOISE_SIGMA_COLOR, BDPT_DENOISE_SIGMA_NORMAL,
                                     BDPT_DENOISE_SIGMA_DEPTH, BDPT_DENOISE_DEMODULATE, 1.f};
            if (windowed) d.norm = static_cast<float>(cfg.spp) / static_cast<float>(window.count);
            std::vector<float> den(px * 3);
            if (bdpt_denoise_host(fctx, cfg.width, cfg.height, rgb.data(), aov.data(), den.data(), &d) != BDPT_OK)
                return die("bdpt_denoise_host");
            const std::string side = side_path(exr, "_denoised");
            if (bdpt_save_exr(den.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
            std::printf("Saved EXR image to %s\n", side.c_str());
            if (display != DISPLAY_NONE) shown_color.swap(den);
        }
        if (want_denoise_var) {
            bdpt_denoise_params d = {denoise_var_iterations, BDPT_DENOISE_VAR_SIGMA_COLOR, BDPT_DENOISE_SIGMA_NORMAL,
                                     BDPT_DENOISE_SIGMA_DEPTH, BDPT_DENOISE_DEMODULATE, 1.f};
            if (windowed) d.norm = static_cast<float>(cfg.spp) / static_cast<float>(window.count);
            std::vector<float> den(px * 3);
            if (bdpt_denoise_var_host(fctx, cfg.width, cfg.height, rgb.data(), variance.data(), aov.data(), den.data(),
                                      nullptr, &d) != BDPT_OK)
                return die("bdpt_denoise_var_host");
            const std::string side = side_path(exr, "_denoised");
            if (bdpt_save_exr(den.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
            std::printf("Saved EXR image to %s\n", side.c_str());
            if (display != DISPLAY_NONE) shown_color.swap(den);
        }
        if (display != DISPLAY_NONE) shown_aov.swap(aov);
        if (fctx != ctx) bdpt_ctx_destroy(fctx);
    }
    uint32_t frame_words[4] = {};  // --exposure auto: the frame's meter words, with which its planes are shown too
    const float window_norm = windowed ? static_cast<float>(cfg.spp) / static_cast<float>(window.count) : 1.f;
    if (display != DISPLAY_NONE) {
        bdpt_ctx* dctx = ctx;  // several devices: the first displays
        if (!dctx && bdpt_ctx_create(scene, devices[0], &dctx) != BDPT_OK) return die("bdpt_ctx_create (display)");
        const bool filtered = !shown_color.empty();  // (a filtered frame is normalised already)
        if (const int rc = write_display(dctx, filtered ? shown_color.data() : rgb.data(), shown_aov.empty() ? nullptr : shown_aov.data(),
                                         nullptr, frame_words, true, filtered ? 1.f : window_norm, exr))
            return rc;
        if (dctx != ctx) bdpt_ctx_destroy(dctx);
    }
    // --layers, --light-groups, --strategies: the frame again as n planes (on several devices the
    // first renders them), one EXR per plane under suffix(plane index), optionally only the planes
    // that are not all zero; then after(context, planes), for what follows the planes. --denoise-planes:
    // the set filtered in one call, each written plane's filtered one beside it.
    const size_t plane = static_cast<size_t>(cfg.width) * cfg.height * 3;
    bool guide_written = want_denoise;  // <out>_denoised.exr: --denoise's, else the first shared set's
    auto write_planes = [&](const char* ctx_what, const char* render_what, size_t n, auto render, auto suffix,
                            bool skip_empty, auto after) -> int {
        bdpt_ctx* pctx = ctx;
        if (!pctx && bdpt_ctx_create(scene, devices[0], &pctx) != BDPT_OK) return die(ctx_what);
        std::vector<float> planes(plane * n, 0.f);
        if (render(pctx, planes.data()) != BDPT_OK) return die(render_what);
        for (size_t k = 0; k < n; k++) {
            const float* const px = planes.data() + plane * k;
            if (skip_empty && std::all_of(px, px + plane, [](float v) { return v == 0.f; })) continue;
            const std::string side = side_path(exr, suffix(static_cast<int>(k)).c_str());
            if (bdpt_save_exr(px, cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
            std::printf("Saved EXR image to %s\n", side.c_str());
            // every plane under the sum frame's exposure and white point, so that the planes stay comparable
            if (display != DISPLAY_NONE)
                if (const int rc = write_display(pctx, px, nullptr, nullptr, frame_words, false, window_norm, side)) return rc;
        }
        if (denoise_planes >= 0) {
            bdpt_denoise_params d = {denoise_iterations, BDPT_DENOISE_SIGMA_COLOR, BDPT_DENOISE_SIGMA_NORMAL,
                                     BDPT_DENOISE_SIGMA_DEPTH, BDPT_DENOISE_DEMODULATE, 1.f};
            if (windowed) d.norm = static_cast<float>(cfg.spp) / static_cast<float>(window.count);
            std::vector<float> aov(plane / 3 * 8, 0.f), den(plane * n), guide;
            if (bdpt_render_aov_host(pctx, &p, win, aov.data()) != BDPT_OK) return die("bdpt_render_aov_host");
            if (denoise_planes == BDPT_DENOISE_PLANES_SHARED && !guide_written) guide.resize(plane);
            if (bdpt_denoise_planes_host(pctx, cfg.width, cfg.height, static_cast<int32_t>(n), planes.data(), aov.data(),
                                         nullptr, denoise_planes, &d, den.data(),
                                         guide.empty() ? nullptr : guide.data()) != BDPT_OK)
                return die("bdpt_denoise_planes_host");
            for (size_t k = 0; k < n; k++) {
                const float* const px = planes.data() + plane * k;
                if (skip_empty && std::all_of(px, px + plane, [](float v) { return v == 0.f; })) continue;
                const std::string side = side_path(exr, (suffix(static_cast<int>(k)) + "_denoised").c_str());
                if (bdpt_save_exr(den.data() + plane * k, cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
                std::printf("Saved EXR image to %s\n", side.c_str());
            }
            if (!guide.empty()) {
                const std::string side = side_path(exr, "_denoised");
                if (bdpt_save_exr(guide.data(), cfg.width, cfg.height, side.c_str()) != BDPT_OK) return die("saveEXR");
                std::printf("Saved EXR image to %s\n", side.c_str());
                guide_written = true;
            }
        }
        if (const int rc = after(pctx, planes.data())) return rc;
        if (pctx != ctx) bdpt_ctx_destroy(pctx);
        return EXIT_SUCCESS;
    };
    auto numbered = [](const char* format, auto... v) {
        char suffix[32];
        std::snprintf(suffix, sizeof suffix, format, v...);
        return std::string(suffix);
    };
    auto nothing = [](bdpt_ctx*, const float*) { return EXIT_SUCCESS; };
    if (cross && layers) {  // group the outer axis, as the library lays the planes out
        const int rc = write_planes(
            "bdpt_ctx_create (light groups x layers)", "bdpt_render_group_layers_host",
            static_cast<size_t>(n_emitters) * layers,
            [&](bdpt_ctx* c, float* fb) { return bdpt_render_group_layers_host(c, &p, win, nullptr, n_emitters, layers, fb); },
            [&](int k) { return numbered(".E%02dL%02d", k / layers, k % layers); }, false, nothing);
        if (rc) return rc;
    }
    if (cross && strategies >= 0) {
        const int n = n_s * n_t;
        const int rc = write_planes(
            "bdpt_ctx_create (light groups x strategies)", "bdpt_render_group_strategies_host",
            static_cast<size_t>(n_emitters) * n,
            [&](bdpt_ctx* c, float* fb) {
                return bdpt_render_group_strategies_host(c, &p, win, nullptr, n_emitters, n_s, n_t, strategies, fb);
            },
            [&](int k) { return numbered(".E%02dS%02dT%02d", k / n, k % n / n_t, k % n_t + 1); }, true, nothing);
        if (rc) return rc;
    }
    if (layers && !cross) {
        const int rc = write_planes(
            "bdpt_ctx_create (layers)", "bdpt_render_layers_host", layers,
            [&](bdpt_ctx* c, float* fb) { return bdpt_render_layers_host(c, &p, win, layers, fb); },
            [&](int l) { return numbered(".L%02d", l); }, false, nothing);
        if (rc) return rc;
    }
    if (light_groups && !cross) {
        const int rc = write_planes(
            "bdpt_ctx_create (light groups)", "bdpt_render_light_groups_host", n_emitters,
            [&](bdpt_ctx* c, float* fb) { return bdpt_render_light_groups_host(c, &p, win, n_emitters, nullptr, fb); },
            [&](int e) { return numbered(".E%02d", e); }, false, nothing);
        if (rc) return rc;
    }
    if (strategies >= 0 && !cross) {
        const size_t n = static_cast<size_t>(n_s) * n_t;
        const int rc = write_planes(
            "bdpt_ctx_create (strategies)", "bdpt_render_strategies_host", n,
            [&](bdpt_ctx* c, float* fb) { return bdpt_render_strategies_host(c, &p, win, n_s, n_t, strategies, fb); },
            [&](int k) { return numbered(".S%02dT%02d", k / n_t, k % n_t + 1); }, true,
            [&](bdpt_ctx* c, const float* planes) {  // the contact sheet, after its planes
                std::vector<float> sheet(plane * n);
                if (bdpt_strategies_sheet_host(c, planes, n_s, n_t, cfg.width, cfg.height, nullptr, sheet.data()) != BDPT_OK)
                    return die("bdpt_strategies_sheet_host");
                const std::string side = side_path(exr, ".strategies");
                if (bdpt_save_exr(sheet.data(), n_s * cfg.width, n_t * cfg.height, side.c_str()) != BDPT_OK)
                    return die("saveEXR");
                std::printf("Saved EXR image to %s\n", side.c_str());
                return EXIT_SUCCESS;
            });
        if (rc) return rc;
    }
    if (multi) bdpt_multi_destroy(multi);
    if (ctx) bdpt_ctx_destroy(ctx);
    bdpt_scene_free(scene);
    return EXIT_SUCCESS;
}

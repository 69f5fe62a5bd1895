// CondUNetTiny's samplers, natively (the reference's models/sde_score_model.py:507-569 reverse SDE, :452-504
// PF-ODE; DPM-Solver++(2M), which the reference does not have): the whole loop of a sampling call is one call
// here.  Host code only: every step is one or two U-Net evaluations (unet.hip) whose last kernel, k_step,
// applies the sampler update.
#include <map>
#include <mutex>
#include <optional>

#include "unet.hpp"

namespace tcx {
namespace {

// Concurrent sampling lanes (TCX_LANES = L > 1, default 1): the batch is split into L contiguous
// groups of images, each an independent sampling chain (GroupNorm is per image, CFG pairs stay
// together) advanced step by step on its own HIP stream, so the HBM-bound passes of one lane
// (GroupNorm apply, upsample, head) can run beside the MFMA-bound convs of another.  The noise
// counters use absolute element offsets: the result is identical to one lane.
// Per host thread (round 6: no process-global sampler state besides the thread-local error string):
// tcx_set_sample_lanes sets the calling thread's lane count, which its later workspace queries and
// sampler calls use; 0 means TCX_LANES from the environment.
thread_local int g_lanes = 0;

struct LaneSync {
    hipStream_t s[4];
    hipEvent_t ev[5];
    bool ok = false;
};

// The lane streams and events of the CURRENT device, created on first use on that device (keyed by
// hipGetDevice, so a process sampling on two devices never enqueues one device's lane work on the
// other's streams) and kept for the process's life; guarded by a mutex for concurrent first calls.
LaneSync* lane_sync() {
    static std::mutex mu;
    static std::map<int, LaneSync> per_dev;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = per_dev.find(dev);
    if (it == per_dev.end()) {
        LaneSync ls;
        bool ok = true;
        // lane 0 runs on the caller's stream, so L lanes use L streams (the box has 4 hardware queues:
        // a fifth stream would share one and serialise)
        ls.s[0] = nullptr;
        for (int i = 1; i < 4; ++i) ok = ok && hipStreamCreateWithFlags(&ls.s[i], hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < 5; ++i) ok = ok && hipEventCreateWithFlags(&ls.ev[i], hipEventDisableTiming) == hipSuccess;
        ls.ok = ok;
        it = per_dev.emplace(dev, ls).first;
    }
    return it->second.ok ? &it->second : nullptr;
}

// Joins sampling lanes 1..L-1 back into the caller's stream on EVERY exit of a sampler: on success
// through join() (errors reported), on an error return from the destructor (best effort), so no lane
// work is left unordered against the caller's later use or release of the workspace.
struct LaneJoin {
    LaneSync* ls = nullptr;
    int L = 0;
    hipStream_t st = nullptr;
    int join() {
        LaneSync* s = ls;
        ls = nullptr;
        if (!s) return TCX_OK;
        int rc = TCX_OK;
        for (int l = 1; l < L; ++l) {
            if (hipEventRecord(s->ev[l], s->s[l]) != hipSuccess || hipStreamWaitEvent(st, s->ev[l], 0) != hipSuccess) {
                set_error("tcx_sample: joining lane %d to the caller's stream failed", l);
                rc = TCX_EHIP;
            }
        }
        return rc;
    }
    ~LaneJoin() {
        if (ls) {
            const std::string keep = tcx_last_error();  // the error being returned stays the reported one
            (void)join();
            set_error("%s", keep.c_str());
        }
    }
};

// Fault injection for the sampler's error paths (tcx_debug_fail_eval): the k-th U-Net evaluation
// after arming returns TCX_EINVAL before launching anything (one shot).  Thread-local: arming it on
// one host thread never fails another thread's evaluations.
thread_local int g_fail_eval = 0;

// Workspace of the samplers (one caller allocation; the library allocates nothing): the U-Net
// evaluations' workspace for the (CFG-doubled) rows under the current lane setting, then the
// conditioning tables of the call's n_steps + 1 step-table rows (and between them, for the PF-ODE the
// drift d and the Euler point x_e, for DPM-Solver++ the history image).
size_t sde_ws_parts(const tcx_unet* net, int B, int H, int W, int n_steps, float guidance, size_t* unet_part) {
    const size_t u = align_up(tcx_unet_workspace_size(net, guidance > 0.f ? 2 * B : B, H, W), 256);
    if (unet_part) *unet_part = u;
    return u + cond_tab_bytes(net, B, n_steps + 1) + 256;
}
size_t ode_ws_parts(const tcx_unet* net, int B, int H, int W, int n_steps, float guidance, size_t* unet_part,
                    size_t* img_part) {
    const size_t im = align_up((size_t)B * H * W * sizeof(float), 256);
    if (img_part) *img_part = im;
    return sde_ws_parts(net, B, H, W, n_steps, guidance, unet_part) + 2 * im;
}
size_t dpmpp_ws_parts(const tcx_unet* net, int B, int H, int W, int n_steps, float guidance, size_t* unet_part,
                      size_t* img_part) {
    const size_t im = align_up((size_t)B * H * W * sizeof(float), 256);
    if (img_part) *img_part = im;
    return sde_ws_parts(net, B, H, W, n_steps, guidance, unet_part) + im;
}

// One lane's share of a sampling call: images [b0, b1), their element offset e = b0 * H * W, the lane's
// slice of the U-Net workspace and its stream.
struct Lane {
    int b0, b1;
    size_t e, ws_bytes;
    char* ws;
    hipStream_t st;
};

// The step loop of the samplers: body(i, lane) for every step-table row i = 0 .. n_steps (the last: the
// final projection), step outer and lane inner, so the lanes' enqueues interleave.  L lanes when the lane
// streams exist and the U-Net workspace [wbase, wbase + ubytes) holds L lane slices, else one lane: the
// caller's stream and the whole workspace, no event, no wait, no join.  who: the sampler, for error texts.
template <class Body>
int step_loop(const char* who, const tcx_unet* net, int B, int H, int W, int n_steps, float guidance, char* wbase,
              size_t ubytes, hipStream_t st, Body body) {
    int L = std::min(lanes_setting(), B);
    const int rows = guidance > 0.f ? 2 * B : B;
    LaneSync* ls = L > 1 ? lane_sync() : nullptr;
    if (!ls || ubytes < (size_t)L * lane_ws_bytes(net, rows, H, W, L)) L = 1;
    const size_t lws = L > 1 ? lane_ws_bytes(net, rows, H, W, L) : ubytes;
    std::optional<LaneJoin> lj;
    if (L > 1) {
        TCX_REQUIRE(hipEventRecord(ls->ev[4], st) == hipSuccess, "%s: event record", who);
        lj.emplace();
        for (int l = 1; l < L; ++l)
            TCX_REQUIRE(hipStreamWaitEvent(ls->s[l], ls->ev[4], 0) == hipSuccess, "%s: stream wait", who);
        lj->ls = ls; lj->L = L; lj->st = st;
    }
    const size_t HW = (size_t)H * W;
    for (int i = 0; i <= n_steps; ++i) {
        for (int l = 0; l < L; ++l) {
            const int b0 = (int)((long long)B * l / L), b1 = (int)((long long)B * (l + 1) / L);
            TCX_TRY(body(i, Lane{b0, b1, (size_t)b0 * HW, lws, wbase + l * lws, l == 0 ? st : ls->s[l]}));
        }
    }
    return lj ? lj->join() : TCX_OK;
}

// what every evaluation of a lane has in common; the samplers' bodies set the step's own fields
EvalArgs lane_eval(const tcx_unet* net, const int64_t* y_cat, const float* y_cont, int H, int W, float guidance,
                   const Lane& lane) {
    EvalArgs a{};
    a.net = net; a.y_cat = y_cat + lane.b0; a.y_cont = y_cont + (size_t)lane.b0 * net->y_cont_dim;
    a.B = lane.b1 - lane.b0; a.H = H; a.W = W; a.guidance = guidance;
    a.ws = lane.ws; a.ws_bytes = lane.ws_bytes; a.stream = lane.st;
    return a;
}

}  // namespace

int lanes_setting() {
    static const int env = env_int("TCX_LANES", 1);
    const int v = g_lanes > 0 ? g_lanes : env;
    return v < 1 ? 1 : (v > 4 ? 4 : v);
}

int injected_failure() {
    if (g_fail_eval <= 0) return TCX_OK;
    if (--g_fail_eval > 0) return TCX_OK;
    set_error("tcx_unet_eval: injected failure (tcx_debug_fail_eval)");
    return TCX_EINVAL;
}

}  // namespace tcx

using namespace tcx;

extern "C" int tcx_set_sample_lanes(int lanes) {
    const int prev = lanes_setting();
    g_lanes = lanes < 0 ? 0 : (lanes > 4 ? 4 : lanes);
    return prev;
}

extern "C" int tcx_debug_fail_eval(int k) {
    g_fail_eval = k < 0 ? 0 : k;
    return TCX_OK;
}

extern "C" size_t tcx_sde_workspace_size(const tcx_unet* net, int B, int H, int W, int n_steps, float guidance) {
    if (!net || B <= 0 || n_steps < 0) return 0;
    return sde_ws_parts(net, B, H, W, n_steps, guidance, nullptr);
}

extern "C" size_t tcx_ode_workspace_size(const tcx_unet* net, int B, int H, int W, int n_steps, float guidance) {
    if (!net || B <= 0 || n_steps < 0) return 0;
    return ode_ws_parts(net, B, H, W, n_steps, guidance, nullptr, nullptr);
}

extern "C" int tcx_sde_sample_shard(const tcx_unet* net, float* x, const int64_t* y_cat, const float* y_cont, int B,
                                    int H, int W, int n_steps, float guidance, const float* scal_table,
                                    const float* noise, uint64_t seed, int flags, uint64_t e_base, void* ws,
                                    size_t ws_bytes, void* stream) {
    TCX_REQUIRE(x && scal_table && n_steps >= 0 && ws, "tcx_sde_sample: bad args");
    TCX_REQUIRE((flags & ~TCX_SAMPLE_X0_HAT) == 0, "tcx_sde_sample: unknown flags %d", flags);
    TCX_TRY(validate(net, B, H, W));
    const int fmode = (flags & TCX_SAMPLE_X0_HAT) ? 5 : 2;
    const size_t img = (size_t)B * H * W;
    size_t ubytes = 0;
    const size_t need = sde_ws_parts(net, B, H, W, n_steps, guidance, &ubytes);
    if (ws_bytes < need) {
        set_error("tcx_sde_sample: workspace too small (%zu < %zu, tcx_sde_workspace_size)", ws_bytes, need);
        return TCX_EWS;
    }
    char* wbase = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    CondMaps cmap;
    TCX_TRY(make_cond_maps(net, scal_table, n_steps + 1, y_cat, y_cont, B, st, wbase + ubytes, cmap));
    return step_loop("tcx_sde_sample", net, B, H, W, n_steps, guidance, wbase, ubytes, st, [&](int i, const Lane& lane) {
        const float* row = scal_table + (size_t)i * TCX_SCAL;
        float* xl = x + lane.e;
        EvalArgs a = lane_eval(net, y_cat, y_cont, H, W, guidance, lane);
        a.x = xl; a.t = row; a.scal = row; a.seed = seed; a.e_base = e_base + lane.e; a.ct = cmap.at(i, lane.b0);
        if (i < n_steps) {  // one Euler-Maruyama step on x
            a.mode = 1; a.step = (uint64_t)i; a.x_inout = xl;
            a.z = noise ? noise + (size_t)i * img + lane.e : nullptr;
        } else {  // final projection -> image written over x
            a.mode = fmode; a.eps_out = xl;
        }
        return unet_eval_impl(a);
    });
}

extern "C" int tcx_sde_sample_ex(const tcx_unet* net, float* x, const int64_t* y_cat, const float* y_cont, int B,
                                 int H, int W, int n_steps, float guidance, const float* scal_table, const float* noise,
                                 uint64_t seed, int flags, void* ws, size_t ws_bytes, void* stream) {
    return tcx_sde_sample_shard(net, x, y_cat, y_cont, B, H, W, n_steps, guidance, scal_table, noise, seed, flags, 0,
                                ws, ws_bytes, stream);
}

extern "C" int tcx_sde_sample(const tcx_unet* net, float* x, const int64_t* y_cat, const float* y_cont, int B, int H,
                              int W, int n_steps, float guidance, const float* scal_table, const float* noise,
                              uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    return tcx_sde_sample_ex(net, x, y_cat, y_cont, B, H, W, n_steps, guidance, scal_table, noise, seed, 0, ws,
                             ws_bytes, stream);
}

extern "C" int tcx_ode_sample_ex(const tcx_unet* net, float* x, const int64_t* y_cat, const float* y_cont, int B,
                                 int H, int W, int n_steps, float guidance, const float* scal_table, int flags, void* ws,
                                 size_t ws_bytes, void* stream) {
    TCX_REQUIRE(x && scal_table && n_steps >= 0 && ws, "tcx_ode_sample: bad args");
    TCX_REQUIRE((flags & ~TCX_SAMPLE_X0_HAT) == 0, "tcx_ode_sample: unknown flags %d", flags);
    TCX_TRY(validate(net, B, H, W));
    const int fmode = (flags & TCX_SAMPLE_X0_HAT) ? 5 : 2;
    size_t ubytes = 0, ibytes = 0;
    const size_t need = ode_ws_parts(net, B, H, W, n_steps, guidance, &ubytes, &ibytes);
    if (ws_bytes < need) {
        set_error("tcx_ode_sample: workspace too small (%zu < %zu, tcx_ode_workspace_size)", ws_bytes, need);
        return TCX_EWS;
    }
    char* wbase = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    // [U-Net workspace][d][x_e][conditioning tables]; a lane takes its images' slices of d / x_e
    float* d = reinterpret_cast<float*>(wbase + ubytes);
    float* xe = reinterpret_cast<float*>(wbase + ubytes + ibytes);
    CondMaps cmap;
    TCX_TRY(make_cond_maps(net, scal_table, n_steps + 1, y_cat, y_cont, B, st, wbase + ubytes + 2 * ibytes, cmap));
    return step_loop("tcx_ode_sample", net, B, H, W, n_steps, guidance, wbase, ubytes, st, [&](int i, const Lane& lane) {
        const float* row = scal_table + (size_t)i * TCX_SCAL;
        float *xl = x + lane.e, *xel = xe + lane.e;
        EvalArgs a = lane_eval(net, y_cat, y_cont, H, W, guidance, lane);
        a.t = row; a.scal = row; a.e_base = lane.e;
        const int stages = i < n_steps ? 2 : 1;  // a Heun step's two evaluations, or the final projection
        for (int s = 0; s < stages; ++s) {
            if (i == n_steps) {  // -> image written over x
                a.mode = fmode; a.x = xl; a.eps_out = xl;
            } else if (s == 0) {  // stage 1 at t_i on x: the drift d and the Euler point x_e
                a.mode = 3; a.x = xl; a.x2 = xel; a.x_inout = xl; a.eps_out = d + lane.e;
            } else {  // stage 2 at t_{i+1} on x_e (table row i + 1, the step's own scal row): x
                a.mode = 4; a.x = xel; a.x2 = nullptr; a.t = row + TCX_SCAL;
            }
            a.ct = cmap.at(i + s, lane.b0);
            TCX_TRY(unet_eval_impl(a));
        }
        return TCX_OK;
    });
}

extern "C" int tcx_ode_sample(const tcx_unet* net, float* x, const int64_t* y_cat, const float* y_cont, int B, int H,
                              int W, int n_steps, float guidance, const float* scal_table, void* ws, size_t ws_bytes,
                              void* stream) {
    return tcx_ode_sample_ex(net, x, y_cat, y_cont, B, H, W, n_steps, guidance, scal_table, 0, ws, ws_bytes, stream);
}

extern "C" size_t tcx_dpmpp_workspace_size(const tcx_unet* net, int B, int H, int W, int n_steps, float guidance) {
    if (!net || B <= 0 || n_steps < 0) return 0;
    return dpmpp_ws_parts(net, B, H, W, n_steps, guidance, nullptr, nullptr);
}

// DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2; tcx.h states the update): one evaluation per step, whose k_step
// applies the first-order (mode 6) or second-order (mode 7) update from the step's coefficient row.
extern "C" int tcx_dpmpp_sample(const tcx_unet* net, float* x, const int64_t* y_cat, const float* y_cont, int B,
                                int H, int W, int n_steps, int order, float guidance, const float* scal_table,
                                const float* coef_table, int flags, void* ws, size_t ws_bytes, void* stream) {
    TCX_REQUIRE(x && scal_table && n_steps >= 0 && ws, "tcx_dpmpp_sample: bad args");
    TCX_REQUIRE(order == 1 || order == 2, "tcx_dpmpp_sample: order must be 1 or 2, got %d", order);
    TCX_REQUIRE((flags & ~(TCX_SAMPLE_X0_HAT | TCX_DPM_LOWER_ORDER_FINAL)) == 0, "tcx_dpmpp_sample: unknown flags %d",
                flags);
    TCX_REQUIRE(coef_table || n_steps == 0, "tcx_dpmpp_sample: null coefficient table");
    TCX_TRY(validate(net, B, H, W));
    const int fmode = (flags & TCX_SAMPLE_X0_HAT) ? 5 : 2;
    const bool lower_final = (flags & TCX_DPM_LOWER_ORDER_FINAL) != 0;
    size_t ubytes = 0, ibytes = 0;
    const size_t need = dpmpp_ws_parts(net, B, H, W, n_steps, guidance, &ubytes, &ibytes);
    if (ws_bytes < need) {
        set_error("tcx_dpmpp_sample: workspace too small (%zu < %zu, tcx_dpmpp_workspace_size)", ws_bytes, need);
        return TCX_EWS;
    }
    char* wbase = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    // [U-Net workspace][history x0][conditioning tables]; a lane takes its images' slice of the history
    float* hist = reinterpret_cast<float*>(wbase + ubytes);
    CondMaps cmap;
    TCX_TRY(make_cond_maps(net, scal_table, n_steps + 1, y_cat, y_cont, B, st, wbase + ubytes + ibytes, cmap));
    return step_loop("tcx_dpmpp_sample", net, B, H, W, n_steps, guidance, wbase, ubytes, st, [&](int i, const Lane& lane) {
        const float* row = scal_table + (size_t)i * TCX_SCAL;
        float* xl = x + lane.e;
        EvalArgs a = lane_eval(net, y_cat, y_cont, H, W, guidance, lane);
        a.x = xl; a.t = row; a.scal = row; a.e_base = lane.e; a.ct = cmap.at(i, lane.b0);
        if (i < n_steps) {  // one multistep update of x, first order where the history is not to be used
            const bool first = order == 1 || i == 0 || (lower_final && i == n_steps - 1);
            a.mode = first ? 6 : 7; a.x_inout = xl; a.coef = coef_table + (size_t)i * TCX_DPM_COEF; a.hist = hist + lane.e;
        } else {  // final projection -> image written over x
            a.mode = fmode; a.eps_out = xl;
        }
        return unet_eval_impl(a);
    });
}

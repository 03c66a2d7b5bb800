// libpam_hip.so, tracker part: the One-Euro filter on the tracks' 3D output (k_one_euro) behind pam_set_one_euro / pam_one_euro, and its
// parity entry pam_op_one_euro.  The step itself is pam_one_euro.hpp; the rules are in include/pam.h.  gfx950 only.
#include <cmath>
#include "pam_tracker.hpp"
#include "pam_one_euro.hpp"

// ---- filter state of one scene (HBM resident across frames, zero = no samples anywhere), by track SLOT ---------------------------------
struct OeState {
    int *id, *last_frame, *n;            // [MAXT] the track the slot's filters belong to, the frame of their newest sample, samples taken
    double *freq, *t_last;               // [MAXT] shared by the 51 channels of a track
    double *x_prev, *x_hat, *dx_hat;     // [MAXT][51]
};
__host__ __device__ inline char* carve_oe(char* base, int MAXT, OeState& s) {
    Carver c{base};
    s.freq = c.take<double>(MAXT); s.t_last = c.take<double>(MAXT);
    s.x_prev = c.take<double>((size_t)MAXT * J3); s.x_hat = c.take<double>((size_t)MAXT * J3); s.dx_hat = c.take<double>((size_t)MAXT * J3);
    s.id = c.take<int>(MAXT); s.last_frame = c.take<int>(MAXT); s.n = c.take<int>(MAXT);
    return c.bytes(0);
}

#define OE_BLOCK 256
#define OE_MAXT 64                       /* pam_create: at most 64 tracks per scene */
enum { OE_RAW = 0, OE_HOLD = 1, OE_DONE = 2, OE_STEP = 3 };     // what a row is: the raw pose, the held x_hat, this frame's x_hat (already taken / taken now)

struct OneEuroArgs {
    Dims d;
    PamOneEuro cfg;
    const char* state; size_t state_stride;
    char* oe; size_t oe_stride;
    int frame_id;
    double* pose; int* meta;
};

// One workgroup per scene.  Pass 1, one lane per list position: the slot, its newest pose and the filter header as it was BEFORE this
// call go to LDS (all 51 channels of a track need the old n, freq and t_last).  Pass 2, a stride loop over (track, channel): the step, or
// a copy.  Pass 3, behind a barrier: the per-slot header and the meta rows.  Reads the tracker state only; plain stores, no atomics.
__global__ __launch_bounds__(OE_BLOCK) void k_one_euro(OneEuroArgs A) {
    __shared__ int s_slot[OE_MAXT], s_newest[OE_MAXT], s_n[OE_MAXT], s_mode[OE_MAXT];
    __shared__ double s_freq[OE_MAXT], s_tlast[OE_MAXT];
    const Dims d = A.d;
    const int MAXT = d.MAXT, HCAP = d.HCAP, tid = threadIdx.x, scene = blockIdx.x;
    SceneState st;
    carve_state(const_cast<char*>(A.state) + (size_t)scene * A.state_stride, d, st);
    OeState oe;
    carve_oe(A.oe + (size_t)scene * A.oe_stride, MAXT, oe);
    double* const pose = A.pose + (size_t)scene * MAXT * J3;
    int* const meta = A.meta + (size_t)scene * (2 + 3 * MAXT);
    const int nT = min(max(st.hdr[0], 0), MAXT);
    const double t = (double)A.frame_id / A.cfg.freq;

    for (int i = tid; i < nT; i += OE_BLOCK) {
        const int s = min(max(st.order[i], 0), MAXT - 1);                       // device state is nobody's to trust: no index leaves the scene
        const int len = st.h_len[s];
        const int newest = len > 0 ? min(max(ring_newest(st, s, HCAP), 0), HCAP - 1) : 0;
        const bool fresh = len > 0 && st.hist_time[s * HCAP + newest] == A.frame_id;
        const bool same = oe.n[s] > 0 && oe.id[s] == st.track_id[s];
        int mode;
        if (!fresh) mode = same ? OE_HOLD : OE_RAW;
        else if (same && oe.last_frame[s] == A.frame_id) mode = OE_DONE;
        else mode = OE_STEP;
        const bool cont = same && !(mode == OE_STEP && A.frame_id < oe.last_frame[s]);      // time went back: the filter starts over
        s_slot[i] = s; s_newest[i] = newest; s_mode[i] = mode;
        s_n[i] = cont ? oe.n[s] : 0;
        s_freq[i] = cont ? oe.freq[s] : A.cfg.freq;
        s_tlast[i] = cont ? oe.t_last[s] : 0.0;
    }
    __syncthreads();

    for (int it = tid; it < MAXT * J3; it += OE_BLOCK) {
        const int i = it / J3, e = it - i * J3;
        double out = 0.0;                                                        // rows from n_tracks on
        if (i < nT) {
            const int s = s_slot[i], mode = s_mode[i];
            const size_t ch = (size_t)s * J3 + e;
            const double x = st.hist[((size_t)s * HCAP + s_newest[i]) * J3 + e];
            if (mode == OE_STEP) {
                double xp = oe.x_prev[ch], xh = oe.x_hat[ch], dh = oe.dx_hat[ch];
                out = one_euro_step(A.cfg, s_n[i], s_freq[i], s_tlast[i], t, x, xp, xh, dh);
                oe.x_prev[ch] = xp; oe.x_hat[ch] = xh; oe.dx_hat[ch] = dh;
            } else {
                out = mode == OE_RAW ? x : oe.x_hat[ch];
            }
        }
        pose[it] = out;
    }
    __syncthreads();

    for (int i = tid; i < MAXT; i += OE_BLOCK) {
        int* m = meta + 2 + 3 * i;
        if (i >= nT) { m[0] = -1; m[1] = 0; m[2] = 0; continue; }
        const int s = s_slot[i], mode = s_mode[i], n = s_n[i];
        if (mode == OE_STEP) {
            oe.id[s] = st.track_id[s]; oe.last_frame[s] = A.frame_id; oe.n[s] = n + 1;
            oe.freq[s] = one_euro_freq(n, s_freq[i], s_tlast[i], t); oe.t_last[s] = t;
        }
        m[0] = st.track_id[s]; m[1] = mode >= OE_DONE ? 1 : 0; m[2] = mode == OE_STEP ? n + 1 : (mode == OE_RAW ? 0 : n);
    }
    if (tid == 0) {
        int fresh = 0;
        for (int i = 0; i < nT; ++i) fresh += s_mode[i] >= OE_DONE;
        meta[0] = nT; meta[1] = fresh;
    }
}

static bool oe_cfg_ok(const PamOneEuro* c) {
    return std::isfinite(c->freq) && std::isfinite(c->mincutoff) && std::isfinite(c->beta) && std::isfinite(c->dcutoff) &&
           c->freq > 0.0 && c->mincutoff > 0.0 && c->dcutoff > 0.0;
}

extern "C" int pam_set_one_euro(PamHandle* h, const PamOneEuro* cfg) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, !cfg || oe_cfg_ok(cfg), "One-Euro configuration: values must be finite, freq, mincutoff and dcutoff > 0");
    if (!cfg && !h->d_oe) return PAM_OK;              // nothing set, nothing to free: no device call
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());                // a k_one_euro in flight still works on the state of before
    if (!cfg) {
        HIPCHK(h, hipFree(h->d_oe));
        h->d_oe = nullptr;
        return PAM_OK;
    }
    if (!h->d_oe) {
        OeState s;
        h->oe_stride = ((size_t)(uintptr_t)carve_oe((char*)0, h->d.MAXT, s) + 255) & ~(size_t)255;
        HIPCHK(h, hipMalloc(&h->d_oe, h->oe_stride * h->d.S));
    }
    HIPCHK(h, hipMemset(h->d_oe, 0, h->oe_stride * h->d.S));
    h->oe = *cfg;
    return PAM_OK;
}

extern "C" int pam_one_euro(PamHandle* h, void* stream, int frame_id, double* dev_pose, int32_t* dev_meta) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, dev_pose && dev_meta, "null output buffer");
    if (!h->d_oe) { h->err = "pam_set_one_euro has not been called"; return PAM_E_STATE; }
    OneEuroArgs A;
    A.d = h->d; A.cfg = h->oe; A.state = h->d_state; A.state_stride = h->state_stride; A.oe = h->d_oe; A.oe_stride = h->oe_stride;
    A.frame_id = frame_id; A.pose = dev_pose; A.meta = dev_meta;
    hipLaunchKernelGGL(k_one_euro, dim3(h->d.S), dim3(OE_BLOCK), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return PAM_OK;
}

// ---- pam_op_one_euro: one lane per channel walks its samples through the step, a new filter each ----------------------------------------
__global__ __launch_bounds__(OE_BLOCK) void k_op_one_euro(PamOneEuro cfg, int n, int K, const double* __restrict__ t,
                                                          const double* __restrict__ x, double* __restrict__ out) {
    const int k = blockIdx.x * OE_BLOCK + threadIdx.x;
    if (k >= K) return;
    double freq = cfg.freq, t_last = 0.0, xp = 0.0, xh = 0.0, dh = 0.0;
    for (int i = 0; i < n; ++i) {
        const double ti = t[i];
        out[(size_t)i * K + k] = one_euro_step(cfg, i, freq, t_last, ti, x[(size_t)i * K + k], xp, xh, dh);
        freq = one_euro_freq(i, freq, t_last, ti); t_last = ti;
    }
}

extern "C" int pam_op_one_euro(PamHandle* h, int n, int K, const double* t, const double* x, const PamOneEuro* cfg, double* out) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, n >= 0 && K >= 1 && K <= 4096, "bad n / K");
    ARGCHK(h, cfg && oe_cfg_ok(cfg), "One-Euro configuration: values must be finite, freq, mincutoff and dcutoff > 0");
    if (n == 0) return PAM_OK;
    ARGCHK(h, t && x && out, "null argument");
    OpStage S(h, __func__);
    const double* dt = S.in(t, n); const double* dx = S.in(x, (size_t)n * K); double* o = S.out<double>((size_t)n * K);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_one_euro, dim3((K + OE_BLOCK - 1) / OE_BLOCK), dim3(OE_BLOCK), 0, 0, *cfg, n, K, dt, dx, o);
    return S.finish(out, o, (size_t)n * K);
}

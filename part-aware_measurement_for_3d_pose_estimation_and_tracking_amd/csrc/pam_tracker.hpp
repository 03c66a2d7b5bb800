// What the tracker's sources share (pam_tracker.hip, pam_frame.hip, pam_track_boxes.hip, pam_track_ops.hip, pam_comm.hip,
// pam_one_euro.hip): the layout of the device-resident scene state and of the per-frame scratch, the handle behind the C ABI of
// include/pam.h, the host-side error macros and the staging helper of the per-operator entry points.  No kernels, and nothing with
// external linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <string>
#include "pam_device.hpp"

using namespace pam;

#define TENTATIVE 1
#define CONFIRMED 2
#define DELETED 3
#define T_NONE (INT_MIN / 2)

struct Dims { int C, MAXP, MAXT, HCAP, MAXH, S, N1, N2; };

struct Carver {
    char* p;
    template <typename T> __host__ __device__ T* take(size_t n) {
        uintptr_t a = (uintptr_t)p;
        const uintptr_t al = sizeof(T) < 8 ? sizeof(T) : 8;
        a = (a + al - 1) & ~(al - 1);
        T* r = (T*)a;
        p = (char*)(a + n * sizeof(T));
        return r;
    }
    __host__ __device__ char* bytes(size_t n) { uintptr_t a = ((uintptr_t)p + 7) & ~(uintptr_t)7; p = (char*)(a + n); return (char*)a; }
};

// ---- per-scene tracker state (HBM resident across frames) -------------------------------------------------------
struct SceneState {
    int* hdr;        // [0] n_tracks [1] next_id [2] status of this frame [3] used_lo [4] used_hi [5] OR of every frame's status since pam_reset
    int* order;      // list position -> slot (the reference's self.tracks order)
    int *track_id, *hits, *age, *tsu, *already, *state, *p2d_n, *h_head, *h_len, *jv_V;
    int* p2d_order;  // [slot][k]   camera ids in dict-insertion order (Appendix A-5)
    int* p2d_time;   // [slot][cid] frame of the stored 2D pose or T_NONE
    int* cur_det;    // [slot][cid] detection index matched in the current frame or -1
    int* hist_time;  // [slot][HCAP] ring
    int* jv_count;   // [slot][17]  kept views per joint of the newest pose
    float* vel;      // [slot][51]  float32 velocity (IterativeTracker.py:391)
    double* p2d_pose;  // [slot][cid][51] rows (y,x,score)
    double* hist;      // [slot][HCAP][51] ring of smoothed poses
};
// ring position of slot s's newest pose
__device__ __forceinline__ int ring_newest(const SceneState& st, int s, int HCAP) { return (st.h_head[s] + st.h_len[s] - 1) % HCAP; }
__host__ __device__ inline char* carve_state(char* base, const Dims& d, SceneState& s) {
    Carver c{base};
    s.hdr = c.take<int>(8);
    s.order = c.take<int>(d.MAXT);
    s.track_id = c.take<int>(d.MAXT); s.hits = c.take<int>(d.MAXT); s.age = c.take<int>(d.MAXT);
    s.tsu = c.take<int>(d.MAXT); s.already = c.take<int>(d.MAXT); s.state = c.take<int>(d.MAXT);
    s.p2d_n = c.take<int>(d.MAXT); s.h_head = c.take<int>(d.MAXT); s.h_len = c.take<int>(d.MAXT);
    s.jv_V = c.take<int>(d.MAXT);
    s.p2d_order = c.take<int>((size_t)d.MAXT * d.C);
    s.p2d_time = c.take<int>((size_t)d.MAXT * d.C);
    s.cur_det = c.take<int>((size_t)d.MAXT * d.C);
    s.hist_time = c.take<int>((size_t)d.MAXT * d.HCAP);
    s.jv_count = c.take<int>((size_t)d.MAXT * J);
    s.vel = c.take<float>((size_t)d.MAXT * J3);
    s.p2d_pose = c.take<double>((size_t)d.MAXT * d.C * J3);
    s.hist = c.take<double>((size_t)d.MAXT * d.HCAP * J3);
    return c.bytes(0);
}

// ---- per-scene scratch (rewritten every frame) -------------------------------------------------------------------
struct Scratch {
    int* misc;       // [0] hyp_n [1] n_tracks at frame start
    int* dt;         // [MAXT]
    double* aff;     // [C][MAXT][MAXP]
    char* lsap1;     // [C] x lsap_scratch_bytes(N1)
    int *as_rows, *as_cols;  // [C][N1]
    int* match_det;  // [MAXT][C] by OLD list position
    unsigned char* taken;  // [C][MAXP]
    int *um_n, *um_idx;    // [C], [C][MAXP]
    int *hyp_size, *hyp_view, *hyp_det;   // [MAXH], [MAXH][C], [MAXH][C]
    double* hc_cost; unsigned char* hc_veto;   // [MAXH][MAXP]
    char* lsap2; int *l2_rows, *l2_cols;
    int *sel_n, *sel_cid, *sel_T;   // [MAXT], [MAXT][C]
    double *pred, *raw3d;           // [MAXT][51]
    uint32_t* conf; double* rayd;   // [MAXT][17][C]
    uint32_t* keep; int* nview; int* ok;   // [MAXT][17], [MAXT][17], [MAXT]
    uint32_t* h_conf; float* h_sum;        // [MAXH][17][C]
    uint32_t* h_keep; double* h_pose; int* h_slot;   // [MAXH][17], [MAXH][51], [MAXH]
    double* rpart;                  // [MAXT][17][DLT_SPLIT][DLT_PACK] partial triangular factors of the split DLT
};
// small, latency-critical arrays first (they are carved out of LDS when they fit: the serial LSAP walks, atomically built
// conflict masks and every index-chasing read then cost an LDS access instead of an L2 round trip), bulk arrays after
__host__ __device__ inline char* carve_ws_hot(char* base, const Dims& d, Scratch& w) {
    Carver c{base};
    w.aff = c.take<double>((size_t)d.C * d.MAXT * d.MAXP);
    w.lsap1 = c.bytes((size_t)d.C * ((lsap_scratch_bytes(d.N1) + 7) & ~(size_t)7));
    w.misc = c.take<int>(8);
    w.dt = c.take<int>(d.MAXT);
    w.as_rows = c.take<int>((size_t)d.C * d.N1); w.as_cols = c.take<int>((size_t)d.C * d.N1);
    w.match_det = c.take<int>((size_t)d.MAXT * d.C);
    w.um_n = c.take<int>(d.C); w.um_idx = c.take<int>((size_t)d.C * d.MAXP);
    w.sel_n = c.take<int>(d.MAXT); w.sel_cid = c.take<int>((size_t)d.MAXT * d.C); w.sel_T = c.take<int>((size_t)d.MAXT * d.C);
    w.conf = c.take<uint32_t>((size_t)d.MAXT * J * d.C);
    w.keep = c.take<uint32_t>((size_t)d.MAXT * J); w.nview = c.take<int>((size_t)d.MAXT * J); w.ok = c.take<int>(d.MAXT);
    w.taken = c.take<unsigned char>((size_t)d.C * d.MAXP);
    return c.bytes(0);
}
__host__ __device__ inline char* carve_ws_bulk(char* base, const Dims& d, Scratch& w) {
    Carver c{base};
    w.hyp_size = c.take<int>(d.MAXH); w.hyp_view = c.take<int>((size_t)d.MAXH * d.C);
    w.hyp_det = c.take<int>((size_t)d.MAXH * d.C);
    w.hc_cost = c.take<double>((size_t)d.MAXH * d.MAXP);
    w.hc_veto = c.take<unsigned char>((size_t)d.MAXH * d.MAXP);
    w.lsap2 = c.bytes(lsap_scratch_bytes(d.N2));
    w.l2_rows = c.take<int>(d.N2); w.l2_cols = c.take<int>(d.N2);
    w.pred = c.take<double>((size_t)d.MAXT * J3); w.raw3d = c.take<double>((size_t)d.MAXT * J3);
    w.rayd = c.take<double>((size_t)d.MAXT * J * d.C);
    w.h_conf = c.take<uint32_t>((size_t)d.MAXH * J * d.C); w.h_sum = c.take<float>((size_t)d.MAXH * J * d.C);
    w.h_keep = c.take<uint32_t>((size_t)d.MAXH * J); w.h_pose = c.take<double>((size_t)d.MAXH * J3);
    w.h_slot = c.take<int>(d.MAXH);
    w.rpart = c.take<double>((size_t)d.MAXT * J * DLT_SPLIT * DLT_PACK);
    return c.bytes(0);
}
__host__ __device__ inline size_t hot_bytes(const Dims& d) {
    Scratch w;
    return ((size_t)(uintptr_t)carve_ws_hot((char*)0, d, w) + 15) & ~(size_t)15;      // offset from a zero base
}
// the bulk arrays start hot_bytes() behind the hot ones: the 16-byte rounded copies of the hot scratch between LDS and its home in
// global memory (launches 1 and 3 of the split step) then never touch hyp_size
__host__ __device__ inline char* carve_ws(char* base, const Dims& d, Scratch& w) {
    carve_ws_hot(base, d, w);
    return carve_ws_bulk(base + hot_bytes(d), d, w);
}
// integer part of the scene state (everything before `vel`): contiguous, copied to LDS for the duration of a frame
__host__ __device__ inline size_t state_int_bytes(const Dims& d) {
    SceneState s;
    carve_state((char*)0, d, s);
    return (size_t)(uintptr_t)(char*)s.vel;
}

// =====================================================================================================================
// Host side of the C ABI
// =====================================================================================================================
struct PamHandle {
    int device = 0;
    Dims d{};
    PamParams prm{};
    PamParams* d_prm = nullptr;
    float *d_P = nullptr, *d_F = nullptr, *d_RK = nullptr; double* d_pos = nullptr;
    bool cams_set = false;
    char* d_state = nullptr; size_t state_stride = 0;
    char* d_ws = nullptr; size_t ws_stride = 0;
    int* d_ndet = nullptr; double* d_det = nullptr;
    int* d_out_i = nullptr; double* d_out_d = nullptr;
    PamOutLayout ol{};
    hipStream_t stream = nullptr;
    char* d_op = nullptr; size_t op_bytes = 0;     // staging for the per-operator entry points
    const int* d_guard = nullptr;                  // pam_set_input_guard
    double* d_lens = nullptr;                      // pam_set_lens: C * PAM_LENS_WORDS doubles while a table is set
    char* d_oe = nullptr; size_t oe_stride = 0;    // pam_set_one_euro: the filter state of every scene (pam_one_euro.hip) while a
    PamOneEuro oe{};                               // configuration is set, and that configuration
    std::string err;
};

#define HIPCHK(h, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    (h)->err = std::string(#call) + ": " + hipGetErrorString(e_); return PAM_E_HIP; } } while (0)
#define ARGCHK(h, cond, msg) do { if (!(cond)) { (h)->err = msg; return PAM_E_ARG; } } while (0)

static inline CamSet camset(const PamHandle* h) { return CamSet{h->d_P, h->d_F, h->d_RK, h->d_pos, h->d.C}; }
// the output record's two sections, over all scenes of the handle (the int32 one is padded to 8 bytes where the float64 one follows it)
static inline size_t out_int_bytes(const PamHandle* h) { return sizeof(int) * (size_t)h->d.S * h->ol.int_words; }
static inline size_t out_dbl_bytes(const PamHandle* h) { return sizeof(double) * (size_t)h->d.S * h->ol.dbl_words; }

// ---- per-operator entry points (pam_op_*): stage to the handle's op buffer, run, copy back -----------------------------------
// An entry point reads: check arguments, stage inputs and outputs, `if (!S.staged()) return PAM_E_ARG;`, launch, `return S.finish(...)`.
namespace {
struct OpStage {
    PamHandle* h; const char* name; size_t off = 0; bool ok = true;
    OpStage(PamHandle* h_, const char* name_) : h(h_), name(name_) { hipSetDevice(h->device); }
    template <typename T> T* in(const T* src, size_t n) {
        T* p = out<T>(n);
        if (p && src && hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return p;
    }
    template <typename T> T* out(size_t n) {
        off = (off + 255) & ~(size_t)255;
        if (off + n * sizeof(T) > h->op_bytes) { ok = false; return nullptr; }
        T* p = (T*)(h->d_op + off); off += n * sizeof(T);
        return p;
    }
    bool staged() { if (!ok) h->err = std::string(name) + ": staging failed"; return ok; }
    template <typename T> void back(T* dst, const T* dev, size_t n) {
        if (hipMemcpy(dst, dev, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) ok = false;
    }
    int done() {
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess || !ok) { h->err = std::string(name) + ": " + (ok ? hipGetErrorString(e) : "staging failed (op buffer too small or copy error)"); return ok ? PAM_E_HIP : PAM_E_ARG; }
        return PAM_OK;
    }
    int status() const { return ok ? PAM_OK : PAM_E_HIP; }
    // wait for the kernel, then copy back every (host destination, device source, count) triple
    template <typename... B> int finish(B... b) { const int rc = done(); if (rc) return rc; backs(b...); return status(); }
    void backs() {}
    template <typename T, typename... R> void backs(T* dst, const T* dev, size_t n, R... r) { back(dst, dev, n); backs(r...); }
};
}  // namespace

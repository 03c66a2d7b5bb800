// libpam_hip.so, tracker part: the handle's life cycle and the plain entry points of the C ABI of include/pam.h.  The per-frame step is
// pam_frame.hip, the boxes from the tracks pam_track_boxes.hip, the per-operator test kernels pam_track_ops.hip, the RCCL exchange
// pam_comm.hip; what they share is pam_tracker.hpp.  gfx950 only.
#include <cmath>
#include "pam_tracker.hpp"
#include "pam_lens.hpp"      // PAM_LENS_WORDS alone (pam_set_lens)

static std::string g_create_err;

extern "C" const char* pam_version(void) { return "pam-hip 0.1 (gfx950)"; }
extern "C" const char* pam_last_error(const PamHandle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int pam_create(PamHandle** out, int device, int n_views, int max_dets, int max_tracks, int max_hyps,
                          int n_scenes, const PamParams* params) {
    if (!out || !params) { g_create_err = "null argument"; return PAM_E_ARG; }
    if (n_views < 1 || n_views > PAM_MAX_VIEWS || max_dets < 1 || max_dets > 32 || max_tracks < 1 || max_tracks > 64 ||
        n_scenes < 1 || params->max_age < 1 || params->max_age > 62 || params->n_taps_body < 1 ||
        params->n_taps_body > PAM_MAX_TAPS || params->n_taps_arm < 1 || params->n_taps_arm > PAM_MAX_TAPS) {
        g_create_err = "capacity out of range (views<=32, dets<=32, tracks<=64, max_age<=62, taps<=16)";
        return PAM_E_ARG;
    }
    PamHandle* h = new PamHandle();
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); delete h; return PAM_E_HIP; }
    Dims& d = h->d;
    d.C = n_views; d.MAXP = max_dets; d.MAXT = max_tracks; d.HCAP = params->max_age + 2;
    d.MAXH = max_hyps > 0 ? max_hyps : 4 * max_dets;
    if (d.MAXH > n_views * max_dets) d.MAXH = n_views * max_dets;
    if (d.MAXH < max_dets) d.MAXH = max_dets;
    d.S = n_scenes;
    d.N1 = max_tracks > max_dets ? max_tracks : max_dets;
    d.N2 = d.MAXH > max_dets ? d.MAXH : max_dets;
    h->prm = *params;
    SceneState st; Scratch ws;
    h->state_stride = ((size_t)(uintptr_t)carve_state((char*)0, d, st) + 255) & ~(size_t)255;
    h->ws_stride = ((size_t)(uintptr_t)carve_ws((char*)0, d, ws) + 255) & ~(size_t)255;
    PamOutLayout& ol = h->ol;
    ol.n_views = d.C; ol.max_dets = d.MAXP; ol.max_tracks = d.MAXT; ol.n_scenes = d.S;
    ol.hdr_words = 4;
    ol.off_order = 10; ol.off_matched = 10 + d.C; ol.off_time2d = 10 + 2 * d.C; ol.off_nviews = 10 + 3 * d.C;
    ol.trk_words = 10 + 3 * d.C + J;
    ol.int_words = ol.hdr_words + d.MAXT * ol.trk_words;
    ol.dbl_hdr_words = 16; ol.dbl_trk_words = 2 * J3;
    ol.dbl_words = ol.dbl_hdr_words + d.MAXT * ol.dbl_trk_words;
    h->op_bytes = 8u << 20;
#define CR(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { g_create_err = std::string(#call) + ": " + hipGetErrorString(e_); \
    pam_destroy(h); return PAM_E_HIP; } } while (0)
    CR(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CR(hipMalloc(&h->d_prm, sizeof(PamParams)));
    CR(hipMemcpy(h->d_prm, params, sizeof(PamParams), hipMemcpyHostToDevice));
    CR(hipMalloc(&h->d_P, sizeof(float) * d.C * 12));
    CR(hipMalloc(&h->d_F, sizeof(float) * d.C * d.C * 9));
    CR(hipMalloc(&h->d_RK, sizeof(float) * d.C * 9));
    CR(hipMalloc(&h->d_pos, sizeof(double) * d.C * 3));
    CR(hipMalloc(&h->d_state, h->state_stride * d.S));
    CR(hipMemset(h->d_state, 0, h->state_stride * d.S));
    CR(hipMalloc(&h->d_ws, h->ws_stride * d.S));
    CR(hipMemset(h->d_ws, 0, h->ws_stride * d.S));
    CR(hipMalloc(&h->d_ndet, sizeof(int) * d.S * d.C));
    CR(hipMalloc(&h->d_det, sizeof(double) * (size_t)d.S * d.C * d.MAXP * J3));
    {   // the record's two sections in ONE allocation, the float64 section behind the int32 one (padded to 8 bytes): a host that lays its
        // pinned landing buffer out the same way gets the record in ONE copy (pam_fetch; Handle.pinned_record)
        const size_t ib = (out_int_bytes(h) + 7) & ~(size_t)7, db = out_dbl_bytes(h);
        char* rec = nullptr;
        CR(hipMalloc(&rec, ib + db));
        CR(hipMemset(rec, 0, ib + db));
        h->d_out_i = (int*)rec; h->d_out_d = (double*)(rec + ib);
    }
    CR(hipMalloc(&h->d_op, h->op_bytes));
#undef CR
    *out = h;
    return PAM_OK;
}

extern "C" int pam_destroy(PamHandle* h) {
    if (!h) return PAM_OK;
    hipSetDevice(h->device);
    hipFree(h->d_prm); hipFree(h->d_P); hipFree(h->d_F); hipFree(h->d_RK); hipFree(h->d_pos);
    hipFree(h->d_state); hipFree(h->d_ws); hipFree(h->d_ndet); hipFree(h->d_det);
    hipFree(h->d_lens); hipFree(h->d_oe);
    hipFree(h->d_out_i); hipFree(h->d_op);                  // (d_out_d lives in d_out_i's allocation)
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return PAM_OK;
}

extern "C" int pam_set_cameras(PamHandle* h, const float* P, const float* F, const float* RK_INV, const double* position) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, P && F && RK_INV && position, "null camera array");
    const Dims& d = h->d;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(h->d_P, P, sizeof(float) * d.C * 12, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_F, F, sizeof(float) * d.C * d.C * 9, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_RK, RK_INV, sizeof(float) * d.C * 9, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_pos, position, sizeof(double) * d.C * 3, hipMemcpyHostToDevice));
    h->cams_set = true;
    return PAM_OK;
}

extern "C" int pam_reset(PamHandle* h) {
    if (!h) return PAM_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemset(h->d_state, 0, h->state_stride * h->d.S));
    if (h->d_oe) HIPCHK(h, hipMemset(h->d_oe, 0, h->oe_stride * h->d.S));      // pam_set_one_euro: every filter starts over with its tracks
    return PAM_OK;
}

extern "C" int pam_out_layout(const PamHandle* h, PamOutLayout* out) {
    if (!h || !out) return PAM_E_ARG;
    *out = h->ol;
    return PAM_OK;
}

// The frame kernel skips a frame (record status bit 16, state untouched) while *dev_word != 0: dev_word is raised by whoever produced
// the frame's keypoints when they are not valid (pam_flag_gate's dev_void).  NULL removes the guard.
extern "C" int pam_set_input_guard(PamHandle* h, const int32_t* dev_word) {
    if (!h) return PAM_E_ARG;
    h->d_guard = dev_word;
    return PAM_OK;
}

// The rig's lens table (pam_lens.hpp), read by k_track_boxes only: NULL, or a table whose every coefficient is exactly zero, removes it.
extern "C" int pam_set_lens(PamHandle* h, const double* lens) {
    if (!h) return PAM_E_ARG;
    const int C = h->d.C;
    bool any = false;
    for (int i = 0; lens && i < C * PAM_LENS_WORDS; ++i) {
        ARGCHK(h, std::isfinite(lens[i]), "non-finite lens table");
        if (i % PAM_LENS_WORDS >= 5 && lens[i] != 0.0) any = true;
    }
    for (int v = 0; lens && any && v < C; ++v)
        ARGCHK(h, lens[v * PAM_LENS_WORDS] != 0.0 && lens[v * PAM_LENS_WORDS + 1] != 0.0, "zero focal length in the lens table");
    if (!any && !h->d_lens) return PAM_OK;             // nothing set, nothing to remove: no device call
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());                 // a k_track_boxes in flight still reads the table of before
    if (!any) {
        HIPCHK(h, hipFree(h->d_lens));
        h->d_lens = nullptr;
        return PAM_OK;
    }
    if (!h->d_lens) HIPCHK(h, hipMalloc(&h->d_lens, sizeof(double) * C * PAM_LENS_WORDS));
    HIPCHK(h, hipMemcpy(h->d_lens, lens, sizeof(double) * C * PAM_LENS_WORDS, hipMemcpyHostToDevice));
    return PAM_OK;
}

extern "C" int pam_fetch(PamHandle* h, void* stream, int32_t* host_out_i, double* host_out_d) {
    if (!h) return PAM_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t ib = (size_t)((char*)h->d_out_d - (char*)h->d_out_i), db = out_dbl_bytes(h);
    if (host_out_i && host_out_d && (char*)host_out_d == (char*)host_out_i + ib) {                 // one landing buffer in the device layout: one copy
        HIPCHK(h, hipMemcpyAsync(host_out_i, h->d_out_i, ib + db, hipMemcpyDeviceToHost, s));
        return PAM_OK;
    }
    if (host_out_i) HIPCHK(h, hipMemcpyAsync(host_out_i, h->d_out_i, out_int_bytes(h), hipMemcpyDeviceToHost, s));
    if (host_out_d) HIPCHK(h, hipMemcpyAsync(host_out_d, h->d_out_d, db, hipMemcpyDeviceToHost, s));
    return PAM_OK;
}

extern "C" int pam_sync(PamHandle* h, void* stream) {
    if (!h) return PAM_E_ARG;
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    return PAM_OK;
}

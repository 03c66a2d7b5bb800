// libpam_hip.so, tracker part: person boxes from the tracker state (k_track_boxes) behind pam_track_boxes.  gfx950 only.
#include "pam_tracker.hpp"
#include "pam_lens.hpp"

// =====================================================================================================================
// Person boxes from the tracker state: every track that was updated at most max_gap frames ago is moved to frame_id by its
// constant-velocity step (k_frame's P4a expression), projected into every view, and boxed.  Output in the detector's layout
// (pam_yolo_detect*), so the boxes are "a detector" to everything downstream.  Reads the state only; one workgroup.
// =====================================================================================================================
#define TB_BLOCK 256
#define TB_CLAMPED 1
struct TrackBoxArgs {
    Dims d;
    CamSet cs;
    const char* state;
    int frame_id, frame_w, frame_h;
    float grow, pad_px, min_size_px;
    int max_gap, max_det;
    float* boxes; int* count; int* ids; int* info;
    const double* lens;    // pam_set_lens: C rows of PAM_LENS_WORDS doubles, or nullptr (the pin-hole rig: the boxes of before, bit for bit)
};
__global__ __launch_bounds__(TB_BLOCK) void k_track_boxes(TrackBoxArgs A) {
    __shared__ float s_box[64 * PAM_MAX_VIEWS][4];          // pam_create: at most 64 tracks x 32 views
    __shared__ unsigned char s_has[64 * PAM_MAX_VIEWS];
    __shared__ int s_clamped;
    const Dims d = A.d;
    const int C = d.C, HCAP = d.HCAP, tid = threadIdx.x;
    SceneState st;
    carve_state(const_cast<char*>(A.state), d, st);
    const int nT = min(max(st.hdr[0], 0), d.MAXT);
    if (tid == 0) s_clamped = 0;
    for (int it = tid; it < C * A.max_det; it += TB_BLOCK) {          // unused rows are defined: zeros, id -1
        for (int e = 0; e < 5; ++e) A.boxes[(size_t)it * 5 + e] = 0.0f;
        if (A.ids) A.ids[it] = -1;
    }
    for (int it = tid; it < nT * C; it += TB_BLOCK) {
        const int i = it / C, v = it % C, s = st.order[i];
        const int newest = ring_newest(st, s, HCAP);
        const int gap = A.frame_id - st.hist_time[s * HCAP + newest];
        bool ok = gap >= 0 && gap <= A.max_gap;
        double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
        if (ok) {
            const float* P = A.cs.P + v * 12;
            const double* hp = st.hist + ((size_t)s * HCAP + newest) * J3;
            const float* vp = st.vel + s * J3;
            for (int j = 0; j < J; ++j) {
                double X[3];
                for (int e = 0; e < 3; ++e) {
                    const float step = vp[j * 3 + e] * (float)gap;                   // float32 product, added in double (P4a)
                    X[e] = hp[j * 3 + e] + (double)step;
                }
                const double h2 = (double)P[8] * X[0] + (double)P[9] * X[1] + (double)P[10] * X[2] + (double)P[11];
                if (!(h2 > 0.0)) { ok = false; break; }                              // a joint behind the camera (or NaN): no box in this view
                double u, w;
                project_point(P, X[0], X[1], X[2], u, w);
                if (A.lens) {                                                        // where the joint lies in the RAW image of this camera
                    const Lens L = lens_row(A.lens, v);
                    if (!lens_is_pinhole(L)) {
                        double x, y, xd, yd;
                        lens_normalise(L, u, w, x, y);
                        lens_forward(L, x, y, xd, yd);
                        lens_pixels(L, xd, yd, u, w);
                    }
                }
                if (j == 0) { x0 = x1 = u; y0 = y1 = w; }
                else { x0 = u < x0 ? u : x0; x1 = u > x1 ? u : x1; y0 = w < y0 ? w : y0; y1 = w > y1 ? w : y1; }
            }
        }
        if (ok) {
            const double cx = 0.5 * (x0 + x1), cy = 0.5 * (y0 + y1);
            const double hx = 0.5 * (double)A.grow * (x1 - x0) + (double)A.pad_px, hy = 0.5 * (double)A.grow * (y1 - y0) + (double)A.pad_px;
            const double bx0 = fmax(cx - hx, 0.0), by0 = fmax(cy - hy, 0.0);
            const double bx1 = fmin(cx + hx, (double)A.frame_w), by1 = fmin(cy + hy, (double)A.frame_h);
            ok = !(bx1 - bx0 < (double)A.min_size_px) && !(by1 - by0 < (double)A.min_size_px) && bx1 == bx1 && by1 == by1 && bx0 == bx0 && by0 == by0;
            s_box[it][0] = (float)bx0; s_box[it][1] = (float)by0; s_box[it][2] = (float)bx1; s_box[it][3] = (float)by1;
        }
        s_has[it] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int v = tid; v < C; v += TB_BLOCK) {                                        // list order within a view: one lane walks it
        int n = 0;
        for (int i = 0; i < nT; ++i) {
            if (!s_has[i * C + v]) continue;
            if (n < A.max_det) {
                float* o = A.boxes + ((size_t)v * A.max_det + n) * 5;
                for (int e = 0; e < 4; ++e) o[e] = s_box[i * C + v][e];
                o[4] = 1.0f;
                if (A.ids) A.ids[v * A.max_det + n] = st.track_id[st.order[i]];
            }
            ++n;
        }
        A.count[v] = min(n, A.max_det); A.count[C + v] = n;
        if (n > A.max_det) atomicOr(&s_clamped, TB_CLAMPED);
    }
    __syncthreads();
    if (tid == 0) {
        int elig = 0;
        for (int i = 0; i < nT; ++i) {
            const int s = st.order[i];
            const int gap = A.frame_id - st.hist_time[s * HCAP + ring_newest(st, s, HCAP)];
            elig += (gap >= 0 && gap <= A.max_gap);
        }
        A.info[0] = s_clamped; A.info[1] = elig;
    }
}

// Person boxes of frame_id from the tracks as the frame launches already on `stream` leave them (k_track_boxes).  Argument errors are
// answered before any device call.
extern "C" int pam_track_boxes(PamHandle* h, void* stream, int scene, int frame_id, int frame_w, int frame_h, float grow, float pad_px,
                               float min_size_px, int max_gap, int max_det, float* dev_boxes, int32_t* dev_count, int32_t* dev_ids,
                               int32_t* dev_info) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, dev_boxes && dev_count && dev_info, "null output buffer");
    ARGCHK(h, max_det >= 1 && max_det <= (1 << 20), "max_det out of range");
    ARGCHK(h, scene >= 0 && scene < h->d.S, "no such scene");
    ARGCHK(h, frame_w >= 0 && frame_h >= 0, "negative frame size");
    if (!h->cams_set) { h->err = "pam_set_cameras has not been called"; return PAM_E_STATE; }
    TrackBoxArgs A;
    A.d = h->d; A.cs = camset(h); A.state = h->d_state + (size_t)scene * h->state_stride;
    A.frame_id = frame_id; A.frame_w = frame_w; A.frame_h = frame_h;
    A.grow = grow; A.pad_px = pad_px; A.min_size_px = min_size_px; A.max_gap = max_gap; A.max_det = max_det;
    A.boxes = dev_boxes; A.count = dev_count; A.ids = dev_ids; A.info = dev_info;
    A.lens = h->d_lens;
    hipLaunchKernelGGL(k_track_boxes, dim3(1), dim3(TB_BLOCK), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return PAM_OK;
}

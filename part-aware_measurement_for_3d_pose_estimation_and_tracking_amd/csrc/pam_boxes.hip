// libpam_hip.so, box lists -> crop table: what connects a detector-layout box tensor (pam_yolo_detect*, pam_track_boxes) to the crop /
// decode kernels without a host trip.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"

#define CT_BLOCK 256
#define CT_MAX_VIEWS 256
#define CT_CUT_VIEW 1     /* info[2]: a view's list was longer than max_dets (or its count lay outside [0, max_det_in]) */
#define CT_CUT_CAP 2      /* info[2]: the views' rows together exceeded cap */

// one detector row (x1, y1, x2, y2, score) -> (x, y, w, h) the way the host path does it: ivclabpose._person_dicts clamps in Python
// floats (max(0, x1), min(x2, w): the comparisons below are Python's, NaN included), subtracts in double, and HRNetPose.predict rounds
// the four numbers to float32 once
__device__ __forceinline__ void box_xywh(const float* __restrict__ row, int frame_w, int frame_h, float* __restrict__ out) {
    const double a = (double)row[0], b = (double)row[1], c = (double)row[2], d = (double)row[3];
    const double x1 = a > 0.0 ? a : 0.0, y1 = b > 0.0 ? b : 0.0;
    const double x2 = (double)frame_w < c ? (double)frame_w : c, y2 = (double)frame_h < d ? (double)frame_h : d;
    out[0] = (float)x1; out[1] = (float)y1; out[2] = (float)(x2 - x1); out[3] = (float)(y2 - y1);
}

// One workgroup: per-view counts -> prefix -> rows.  Rows [total, cap) repeat row total - 1 (or the whole frame of view 0 when there is
// none), so that crop, forward and decode can be launched for cap rows by a host that never learns the count.
__global__ __launch_bounds__(CT_BLOCK) void k_crop_table(int n_views, const int* __restrict__ views, const float* __restrict__ boxes,
                                                         const int* __restrict__ count, int max_det_in, int frame_w, int frame_h,
                                                         int max_dets, int cap, int* __restrict__ view_of, int* __restrict__ slot_of,
                                                         float* __restrict__ xywh, int* __restrict__ n_det, int* __restrict__ info) {
    __shared__ int s_keep[CT_MAX_VIEWS], s_start[CT_MAX_VIEWS], s_src[CT_MAX_VIEWS];
    __shared__ int s_bits, s_total, s_last_view;
    const int tid = threadIdx.x;
    if (tid == 0) s_bits = 0;
    __syncthreads();
    for (int i = tid; i < n_views; i += CT_BLOCK) {
        const int g = views ? views[i] : i;
        const int raw = count[g];
        const int have = min(max(raw, 0), max_det_in);          // device counts are nobody's to trust: no row index leaves the list
        const int k = min(have, max_dets);
        if (raw != k) atomicOr(&s_bits, CT_CUT_VIEW);
        s_keep[i] = k; s_src[i] = g;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0, last = -1;
        long long wanted = 0;
        for (int i = 0; i < n_views; ++i) {
            const int k = min(s_keep[i], cap - run);                // rows are ordered by (view, slot): the first cap of them stay
            wanted += s_keep[i];
            s_start[i] = run; s_keep[i] = k; run += k;
            if (k > 0) last = i;
            n_det[i] = k;
        }
        int bits = s_bits;
        if (wanted > (long long)cap) bits |= CT_CUT_CAP;
        s_total = run; s_last_view = last;
        info[0] = run; info[1] = (int)wanted; info[2] = bits; info[3] = 0;
    }
    __syncthreads();
    const int total = s_total;
    for (int it = tid; it < n_views * max_dets; it += CT_BLOCK) {
        const int i = it / max_dets, s = it % max_dets;
        if (s >= s_keep[i]) continue;
        const int r = s_start[i] + s;                               // < total <= cap
        view_of[r] = i; slot_of[r] = s;
        box_xywh(boxes + ((size_t)s_src[i] * max_det_in + s) * 5, frame_w, frame_h, xywh + (size_t)r * 4);
    }
    const int lv = s_last_view;
    for (int r = total + tid; r < cap; r += CT_BLOCK) {
        if (lv < 0) {
            view_of[r] = 0; slot_of[r] = 0;
            xywh[(size_t)r * 4] = 0.0f; xywh[(size_t)r * 4 + 1] = 0.0f;
            xywh[(size_t)r * 4 + 2] = (float)(double)frame_w; xywh[(size_t)r * 4 + 3] = (float)(double)frame_h;
        } else {
            const int s = s_keep[lv] - 1;
            view_of[r] = lv; slot_of[r] = s;
            box_xywh(boxes + ((size_t)s_src[lv] * max_det_in + s) * 5, frame_w, frame_h, xywh + (size_t)r * 4);
        }
    }
}

extern "C" int pam_crop_table(void* stream, int n_views, const int32_t* dev_views, const float* dev_boxes, const int32_t* dev_count,
                              int max_det_in, int frame_w, int frame_h, int max_dets, int cap, int32_t* dev_view_of,
                              int32_t* dev_slot_of, float* dev_xywh, int32_t* dev_n_det, int32_t* dev_info) {
    if (!dev_boxes || !dev_count || !dev_view_of || !dev_slot_of || !dev_xywh || !dev_n_det || !dev_info) return PAM_E_ARG;
    if (n_views < 1 || n_views > CT_MAX_VIEWS || max_det_in < 1 || max_dets < 1 || cap < 1 || frame_w < 0 || frame_h < 0) return PAM_E_ARG;
    if ((long long)n_views * max_dets > (1ll << 30)) return PAM_E_ARG;
    hipLaunchKernelGGL(k_crop_table, dim3(1), dim3(CT_BLOCK), 0, (hipStream_t)stream, n_views, dev_views, dev_boxes, dev_count,
                       max_det_in, frame_w, frame_h, max_dets, cap, dev_view_of, dev_slot_of, dev_xywh, dev_n_det, dev_info);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

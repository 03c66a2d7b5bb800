// libpam_hip.so, lens distortion out of the decoded keypoints before the tracker sees them: the inverse of the Brown-Conrady model
// (pam_lens.hpp), in float64, in place on the decode's buffer.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_lens.hpp"

#define LN_BLOCK 256
#define LN_MAX 32         /* rows of a view, as pam_pose_nms takes them */
#define LN_J 17
#define LN_ROW (LN_J * 3) /* doubles of a row: (y, x, score)[17] */

// One lane = one keypoint of one slot; lanes of slots at or beyond their view's count, and of pin-hole cameras, leave without a store.
// A latency-bound launch: 10 table doubles and 2 coordinates in, 8 Newton steps (3 float64 divisions each), 2 coordinates out.  info[0]
// has been zeroed on the stream in front of the launch (pam_undistort_keypoints).
__global__ __launch_bounds__(LN_BLOCK) void k_undistort_keypoints(int n_views, int max_dets, int det_slots, double* __restrict__ det,
                                                                  const int* __restrict__ n_det, const int* __restrict__ views,
                                                                  const double* __restrict__ lens, int* __restrict__ info) {
    const int idx = blockIdx.x * LN_BLOCK + threadIdx.x;                // < n_views * 32 * 17: the entry point bounds n_views
    if (idx == 0) {
        int pts = 0;
        for (int v = 0; v < n_views; ++v) pts += min(max(n_det[v], 0), max_dets) * LN_J;
        info[1] = pts;
    }
    if (idx >= n_views * max_dets * LN_J) return;
    const int v = idx / (max_dets * LN_J), rem = idx - v * (max_dets * LN_J), s = rem / LN_J, j = rem - s * LN_J;
    const int n = min(max(n_det[v], 0), max_dets);                      // device counts are nobody's to trust: no row index leaves the view
    if (s >= n) return;
    const pam::Lens L = pam::lens_row(lens, views ? views[v] : v);
    if (pam::lens_is_pinhole(L)) return;
    double* const p = det + ((size_t)v * det_slots + s) * LN_ROW + j * 3;       // (y, x, score): the score is not even read
    const double py = p[0], px = p[1];
    bool ok = isfinite(py) && isfinite(px);
    double dx, dy, x, y, u, w;
    pam::lens_normalise(L, px, py, dx, dy);
    ok = pam::lens_inverse(L, dx, dy, x, y) && ok;
    pam::lens_pixels(L, x, y, u, w);
    if (ok) { p[0] = w; p[1] = u; }
    else atomicAdd(&info[0], 1);                                        // the point keeps its input coordinates
}

extern "C" int pam_undistort_keypoints(void* stream, int n_views, int max_dets, int det_slots, double* dev_det, const int32_t* dev_n_det,
                                       const int32_t* dev_views, const double* dev_lens, int32_t* dev_info) {
    if (!dev_det || !dev_n_det || !dev_lens || !dev_info) return PAM_E_ARG;
    if (n_views < 1 || n_views > (1 << 20) || max_dets < 1 || max_dets > LN_MAX || det_slots < max_dets) return PAM_E_ARG;
    if (hipMemsetAsync(dev_info, 0, 2 * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return PAM_E_HIP;
    const int lanes = n_views * max_dets * LN_J;
    hipLaunchKernelGGL(k_undistort_keypoints, dim3((lanes + LN_BLOCK - 1) / LN_BLOCK), dim3(LN_BLOCK), 0, (hipStream_t)stream, n_views,
                       max_dets, det_slots, dev_det, dev_n_det, dev_views, dev_lens, dev_info);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

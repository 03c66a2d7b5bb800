// libpam_hip.so, duplicate 2D poses out of each view before the tracker sees them: the rescoring + greedy OKS-NMS of the HRNet / Simple
// Baselines test protocol (TEST.OKS_THRE / TEST.IN_VIS_THRE), in float64, in place on the decode's buffer.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"

#define PN_BLOCK 256
#define PN_MAX 32         /* rows of a view: one bit each in the kills / alive / keep words */
#define PN_J 17
#define PN_ROW (PN_J * 3) /* doubles of a row: (y, x, score)[17] */

struct PnVars { double v[PN_J]; };

// One workgroup = one view.  The view's n <= 32 rows, their crop areas and scores are in LDS before anything is stored (the compaction moves
// rows DOWN over rows that other lanes still have to read: the barrier between the last read and the first store is what makes the step
// safe in place).  A latency-bound launch: rank by counting (one lane per row), the n (n - 1) / 2 pairs dealt over the lanes (17 double
// exps each, one bit per direction in a 32 x 32-bit matrix), the greedy walk on bit masks in one lane, the offsets by popcount.
__global__ __launch_bounds__(PN_BLOCK) void k_pose_nms(int max_dets, int det_slots, double* __restrict__ det, const int* __restrict__ n_det_in,
                                                       int n_rows, const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                       const float* __restrict__ xywh, const float* __restrict__ score, long long view_stride,
                                                       long long slot_stride, const int* __restrict__ views, PnVars vars, double oks_thre,
                                                       double in_vis_thre, int* __restrict__ n_det_out, int* __restrict__ keep_from,
                                                       double* __restrict__ pose_score) {
    __shared__ double s_det[PN_MAX * PN_ROW];
    __shared__ double s_area[PN_MAX], s_score[PN_MAX];
    __shared__ unsigned s_kills[PN_MAX];
    __shared__ int s_order[PN_MAX], s_src[PN_MAX];
    __shared__ unsigned s_keep;
    const int tid = threadIdx.x, v = blockIdx.x;
    const int n = min(max(n_det_in[v], 0), max_dets);              // device counts are nobody's to trust: no row index leaves the view
    double* const base = det + (size_t)v * det_slots * PN_ROW;
    if (tid < PN_MAX) { s_area[tid] = 0.0; s_kills[tid] = 0u; s_src[tid] = -1; }
    for (int i = tid; i < n * PN_ROW; i += PN_BLOCK) s_det[i] = base[i];
    __syncthreads();
    // the boxes that produced the rows: crop rows of this view (repeats of a (view, slot) carry the same box and store the same bits)
    for (int r = tid; r < n_rows; r += PN_BLOCK) {
        if (view_of[r] != v) continue;
        const int s = slot_of[r];
        if (s < 0 || s >= n) continue;
        s_area[s] = (double)xywh[(size_t)r * 4 + 2] * (double)xywh[(size_t)r * 4 + 3];
    }
    if (tid < n) {
        double sum = 0.0;
        int cnt = 0;
        for (int j = 0; j < PN_J; ++j) {
            const double s = s_det[tid * PN_ROW + j * 3 + 2];
            if (s > in_vis_thre) { sum += s; ++cnt; }                // (NaN and -inf fail the comparison)
        }
        const double mean = cnt ? sum / (double)cnt : 0.0;
        const long long g = views ? views[v] : v;
        const double b = score ? (double)score[g * view_stride + (long long)tid * slot_stride] : 1.0;
        s_score[tid] = b * mean;
    }
    __syncthreads();
    if (tid < n) {                                                  // descending score, equal scores by lower slot; a NaN score goes last
        const double mine = s_score[tid] == s_score[tid] ? s_score[tid] : -INFINITY;
        int rank = 0;
        for (int k = 0; k < n; ++k) {
            const double other = s_score[k] == s_score[k] ? s_score[k] : -INFINITY;
            rank += (other > mine || (other == mine && k < tid)) ? 1 : 0;
        }
        s_order[rank] = tid;
    }
    const int n_pairs = n * (n - 1) / 2;
    for (int t = tid; t < n_pairs; t += PN_BLOCK) {
        int p = 0, rem = t;
        while (rem >= n - 1 - p) { rem -= n - 1 - p; ++p; }          // pair t of the upper triangle, row by row
        const int q = p + 1 + rem;
        const double* a = s_det + p * PN_ROW;
        const double* c = s_det + q * PN_ROW;
        const double den = (s_area[p] + s_area[q]) / 2.0 + 2.220446049250313e-16;
        double acc = 0.0;
        for (int j = 0; j < PN_J; ++j) {
            const double dy = a[j * 3] - c[j * 3], dx = a[j * 3 + 1] - c[j * 3 + 1];
            const double e = (dx * dx + dy * dy) / vars.v[j] / den / 2.0;
            acc += exp(-e);
        }
        if (acc / (double)PN_J > oks_thre) {                          // (a NaN OKS kills nothing)
            atomicOr(&s_kills[p], 1u << q);
            atomicOr(&s_kills[q], 1u << p);
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned alive = n >= 32 ? 0xffffffffu : ((1u << n) - 1u), keep = 0u;
        for (int r = 0; r < n; ++r) {
            const int i = s_order[r];
            if (!((alive >> i) & 1u)) continue;
            keep |= 1u << i;
            alive &= ~(s_kills[i] | (1u << i));                      // only what the KEPT row kills dies: not transitive
        }
        s_keep = keep;
    }
    __syncthreads();
    const unsigned keep = s_keep;
    const int kept = __popc(keep);
    if (tid < n && ((keep >> tid) & 1u)) s_src[__popc(keep & ((1u << tid) - 1u))] = tid;     // kept rows stay in slot order
    __syncthreads();
    for (int i = tid; i < n * PN_ROW; i += PN_BLOCK) {
        const int d = i / PN_ROW;
        base[i] = d < kept ? s_det[s_src[d] * PN_ROW + (i - d * PN_ROW)] : 0.0;
    }
    if (tid < max_dets) {
        const int src = tid < kept ? s_src[tid] : -1;
        keep_from[(size_t)v * max_dets + tid] = src;
        pose_score[(size_t)v * max_dets + tid] = src >= 0 ? s_score[src] : 0.0;
    }
    if (tid == 0) n_det_out[v] = kept;
}

extern "C" int pam_pose_nms(void* stream, int n_views, int max_dets, int det_slots, double* dev_det, const int32_t* dev_n_det_in, int n_rows,
                            const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_xywh, const float* dev_score,
                            long long view_stride, long long slot_stride, const int32_t* dev_views, const double* vars, double oks_thre,
                            double in_vis_thre, int32_t* dev_n_det_out, int32_t* dev_keep_from, double* dev_pose_score) {
    if (!dev_det || !dev_n_det_in || !dev_view_of || !dev_slot_of || !dev_xywh || !vars || !dev_n_det_out || !dev_keep_from || !dev_pose_score)
        return PAM_E_ARG;
    if (n_views < 1 || max_dets < 1 || max_dets > PN_MAX || det_slots < max_dets || n_rows < 0) return PAM_E_ARG;
    if (dev_n_det_out == dev_n_det_in) return PAM_E_ARG;            // a forward that is issued again filters from the ORIGINAL counts
    PnVars pv;
    for (int j = 0; j < PN_J; ++j) pv.v[j] = vars[j];
    hipLaunchKernelGGL(k_pose_nms, dim3(n_views), dim3(PN_BLOCK), 0, (hipStream_t)stream, max_dets, det_slots, dev_det, dev_n_det_in, n_rows,
                       dev_view_of, dev_slot_of, dev_xywh, dev_score, view_stride, slot_stride, dev_views, pv, oks_thre, in_vis_thre,
                       dev_n_det_out, dev_keep_from, dev_pose_score);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

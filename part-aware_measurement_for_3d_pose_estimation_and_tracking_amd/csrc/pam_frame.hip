// libpam_hip.so, tracker part: the fused per-frame kernel (one workgroup per scene), how it is launched on a handle, and the frame
// entry points of the C ABI of include/pam.h.  gfx950 only.
#include <stdio.h>
#include <stdlib.h>
#include "pam_tracker.hpp"

#define ST_TRACK_OVERFLOW 1
#define ST_HYP_OVERFLOW 2
#define ST_LSAP_INFEASIBLE 4
#define ST_NDET_CLAMPED 8       /* a per-view detection count outside [0, max_dets] was clamped (pam_frame_dev takes device counts unchecked) */
#define ST_INPUT_VOID 16        /* the producer of this frame's keypoints declared them void (pam_set_input_guard / the records' void flag): the
                                   frame was NOT applied -- state untouched, record without tracks, out_i[3] = first void frame of the run of void frames */
#define BLOCK 256

struct FrameArgs {
    Dims d;
    CamSet cs;
    const PamParams* prm;
    char* state; size_t state_stride;
    char* ws; size_t ws_stride;
    const int* n_det; const double* det;
    const int* view_row;   // view-sharded input (pam_frame_dev_views): det = the all-gathered records, view v's record is row view_row[v];
                           // record = (MAXP + 1) x 51 doubles: MAXP detection rows, then the view's detection count in the first double
    int* out_i; double* out_d;
    PamOutLayout ol;
    int frame_id;
    int hot_in_lds;
    const int* guard;      // pam_set_input_guard: a device word the producer of the keypoints raises when they are void (pam_flag_gate's dev_void)
};

__device__ const int g_zeroT[PAM_MAX_VIEWS] = {0};

__device__ __forceinline__ double now_s() { return (double)__builtin_amdgcn_s_memrealtime() * 1e-8; }

// =====================================================================================================================
// The per-frame step: IterativeTracker.tracking (IterativeTracker.py:115-180) + output collection
// (ivclabpose.py:259-287).  One 256-thread workgroup per scene; phases separated by workgroup barriers.
// =====================================================================================================================
// PART: 0 = the whole step in one launch.  Rigs with more than 8 cameras run it as THREE launches (round 6): 1 = P0-P4a (association,
// view selection), 2 = P4b (the epipolar conflict sets: nT x V(V-1)/2 x 17 independent items -- 55 000 on the 31-camera rig, which one
// workgroup walked in 54 passes of dependent L2 loads, 136 of its 297 us) spread over MANY workgroups, 3 = P4c-P7.  Launch 2 works on
// the global copy of the scratch and state; launches 1 and 3 hold them in LDS when they fit (hot_in_lds); one scene per handle.
template <int NTHREADS, int PART = 0>
__global__ __launch_bounds__(NTHREADS, 4) void k_frame(FrameArgs A) {      // 4 waves per SIMD: four 256-thread scenes per CU (<= 128 VGPRs)
    const Dims d = A.d;
    const int C = d.C, MAXP = d.MAXP, MAXT = d.MAXT, HCAP = d.HCAP, MAXH = d.MAXH;
    const int sidx = PART == 2 ? 0 : blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    // P4b's items are dealt over the whole grid in the split form
    const int it0 = PART == 2 ? (int)blockIdx.x * (int)blockDim.x + tid : tid, itS = PART == 2 ? (int)(gridDim.x * blockDim.x) : NT;
    SceneState st; Scratch ws;
    carve_state(A.state + (size_t)sidx * A.state_stride, d, st);
    carve_ws(A.ws + (size_t)sidx * A.ws_stride, d, ws);
    extern __shared__ __attribute__((aligned(16))) char hot_lds[];
    char* const st_glob = A.state + (size_t)sidx * A.state_stride;
    const size_t st_ints = state_int_bytes(d);
    // ---- input guard: keypoints whose producer gave up (a device-side gate of the captured HRNet forward timed out, csrc/pam_sync.hip)
    //      must never reach the tracker state -- the reference's PersonPoseDetect (/root/reference/src/ivclabpose.py:208-212) cannot hand
    //      out a frame it later disowns.  The word is raised on THIS device (A.guard) or travels with a view-sharded record (second double
    //      of its count row, set by the rank that produced it).  A void frame leaves the state as it is; hdr[6] remembers the first frame
    //      of the current run of void frames (+ 1) so that the host knows where to resume.
    if (PART >= 2) {                                     // the split step decides ONCE, in its first launch (the word may rise between the launches)
        if (ws.misc[2]) return;
    } else {
        int voided = A.guard ? __hip_atomic_load(A.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        if (A.view_row)
            for (int v = 0; v < d.C; ++v) voided |= (A.det[((size_t)A.view_row[v] * (d.MAXP + 1) + d.MAXP) * J3 + 1] != 0.0);
        if (PART == 1 && threadIdx.x == 0) ws.misc[2] = voided;
        if (voided) {
            if (threadIdx.x == 0) {
                int* oi = A.out_i + (size_t)sidx * A.ol.int_words;
                double* od = A.out_d + (size_t)sidx * A.ol.dbl_words;
                if (st.hdr[6] == 0) st.hdr[6] = A.frame_id + 1;
                oi[0] = 0; oi[1] = ST_INPUT_VOID | (st.hdr[5] << 16); oi[2] = A.frame_id; oi[3] = st.hdr[6] - 1;
                const double t = now_s();
                for (int k = 0; k < 12; ++k) od[k] = t;
            }
            return;
        }
    }
    char* const ws_glob = A.ws + (size_t)sidx * A.ws_stride;         // the hot scratch's home in global memory (between the launches of a split step)
    if (A.hot_in_lds) {
        carve_ws_hot(hot_lds, d, ws);                                   // small scratch in LDS
        char* st_lds = hot_lds + hot_bytes(d);                          // integer scene state in LDS for this frame
        for (size_t o = (size_t)threadIdx.x * 4; o < st_ints; o += (size_t)blockDim.x * 4) *(int*)(st_lds + o) = *(const int*)(st_glob + o);
        if (PART == 3)                                                  // ... and what the first two launches left in the hot scratch
            for (size_t o = (size_t)threadIdx.x * 4; o < hot_bytes(d); o += (size_t)blockDim.x * 4) *(int*)(hot_lds + o) = *(const int*)(ws_glob + o);
        const ptrdiff_t sh = st_lds - st_glob;
#define REBASE(p) p = (int*)((char*)(p) + sh)
        REBASE(st.hdr); REBASE(st.order); REBASE(st.track_id); REBASE(st.hits); REBASE(st.age); REBASE(st.tsu); REBASE(st.already);
        REBASE(st.state); REBASE(st.p2d_n); REBASE(st.h_head); REBASE(st.h_len); REBASE(st.jv_V); REBASE(st.p2d_order);
        REBASE(st.p2d_time); REBASE(st.cur_det); REBASE(st.hist_time); REBASE(st.jv_count);
#undef REBASE
        if (PART == 1 && threadIdx.x == 0) ws.misc[2] = 0;               // (the LDS copy goes home at the end of this launch: not void, see above)
        __syncthreads();
    }
    const PamParams& prm = *A.prm;
    const CamSet cs = A.cs;
    const int frame = A.frame_id;
    const int* vrow = A.view_row;                                       // non-null: records gathered from the ranks (one scene)
    const int* n_det = vrow ? nullptr : A.n_det + (size_t)sidx * C;
    const double* det = vrow ? A.det : A.det + (size_t)sidx * C * MAXP * J3;
    const size_t recd = vrow ? (size_t)(MAXP + 1) * J3 : (size_t)MAXP * J3;
    int* out_i = A.out_i + (size_t)sidx * A.ol.int_words;
    double* out_d = A.out_d + (size_t)sidx * A.ol.dbl_words;
#define DET(v, k) (det + (size_t)(vrow ? vrow[v] : (v)) * recd + (size_t)(k) * J3)
    // view-sharded records carry the count as a double: a non-finite or out-of-range value is clamped explicitly (never cast: the
    // conversion of a NaN is undefined) and raises ST_NDET_CLAMPED below
    auto rec_count = [&](int v) -> double { return det[(size_t)vrow[v] * recd + (size_t)MAXP * J3]; };
    auto count_of = [&](int v) -> int {
        if (!vrow) return n_det[v];
        const double c = rec_count(v);
        return (c >= 0.0 && c <= (double)MAXP) ? (int)c : (c > (double)MAXP ? MAXP + 1 : -1);
    };
    const int nT = st.hdr[0];
    // device-side counts are not validated by the host (pam_frame_dev): clamp them so that no index leaves det / ws.taken
#define NDET(v) min(max(count_of(v), 0), MAXP)

    if (PART <= 1) {
    // ---- P0: add_age, time gaps (IterativeTracker.py:126-129) -------------------------------------------------------
    if (tid == 0) {
        out_d[0] = now_s(); ws.misc[1] = nT;
        int bad = 0;
        for (int v = 0; v < C; ++v) { const int nv = count_of(v); bad |= (nv < 0 || nv > MAXP); }
        st.hdr[2] = bad ? ST_NDET_CLAMPED : 0;                       // the status word is per frame (out_i[1]); nothing sticks
    }
    __syncthreads();
    for (int i = tid; i < nT; i += NT) {
        const int s = st.order[i];
        st.already[s] = 0; st.age[s] += 1; st.tsu[s] += 1;
        const int newest = ring_newest(st, s, HCAP);
        ws.dt[i] = frame - st.hist_time[s * HCAP + newest];
        for (int v = 0; v < C; ++v) st.cur_det[s * C + v] = -1;
    }
    for (int k = tid; k < MAXT * C; k += NT) ws.match_det[k] = -1;
    for (int k = tid; k < C * MAXP; k += NT) ws.taken[k] = 0;
    __syncthreads();

    // ---- P1: re-projection affinity for every (view, track, detection) (:137-149) ----------------------------------
    if (MAXP == 8 || MAXP == 16 || MAXP == 32) {
        // the MAXP slots of a (view, track) pair sit in MAXP neighbouring lanes: the track's 17 re-projections are computed once per
        // group and shared through the wave (track_det_affinity_group) instead of once per detection; whole waves iterate together
        const int total = C * nT * MAXP;
        for (int it = tid; it - (tid & 63) < total; it += NT) {
            const bool in = it < total;
            const int ic = in ? it : 0;
            const int v = ic / (nT * MAXP), r = ic % (nT * MAXP), i = r / MAXP, k = r % MAXP;
            const bool live = in && k < NDET(v);
            const int s = st.order[i];
            const int newest = ring_newest(st, s, HCAP);
            const int dt = ws.dt[i];
            const double e = (dt >= 0 && dt < PAM_EXP_TABLE) ? prm.exp_lambda_a[dt] : exp(prm.lambda_a * (double)dt);
            const float* Pv = cs.P + v * 12;
            const double* X3 = st.hist + ((size_t)s * HCAP + newest) * J3;
            const double* dk = DET(v, live ? k : 0);
            const double a = MAXP == 8 ? track_det_affinity_group<8>(Pv, X3, dk, prm.alpha2d * (double)dt, e, prm.count_gate, live)
                           : MAXP == 16 ? track_det_affinity_group<16>(Pv, X3, dk, prm.alpha2d * (double)dt, e, prm.count_gate, live)
                                        : track_det_affinity_group<32>(Pv, X3, dk, prm.alpha2d * (double)dt, e, prm.count_gate, live);
            if (live) ws.aff[((size_t)v * MAXT + i) * MAXP + k] = a;
        }
    } else
    for (int it = tid; it < C * nT * MAXP; it += NT) {
        const int v = it / (nT * MAXP), r = it % (nT * MAXP), i = r / MAXP, k = r % MAXP;
        if (k >= NDET(v)) continue;
        const int s = st.order[i];
        const int newest = ring_newest(st, s, HCAP);
        const int dt = ws.dt[i];
        const double e = (dt >= 0 && dt < PAM_EXP_TABLE) ? prm.exp_lambda_a[dt] : exp(prm.lambda_a * (double)dt);
        ws.aff[((size_t)v * MAXT + i) * MAXP + k] =
            track_det_affinity(cs.P + v * 12, st.hist + ((size_t)s * HCAP + newest) * J3, DET(v, k),
                               prm.alpha2d * (double)dt, e, prm.count_gate);
    }
    __syncthreads();
#ifdef PAM_FINE_STAMPS
    if (tid == 0) out_d[12] = now_s();
#endif

    // ---- P2: one assignment problem per view (:150-160) ---------------------------------------------------------
    // one WAVE per view (lsap_solve_wave: a lane per column / row), views dealt over the workgroup's waves
    for (int v = tid >> 6; v < C; v += NT >> 6) {
        const int m = NDET(v);
        if (nT > 0 && m > 0) {
            int* rows = ws.as_rows + v * d.N1; int* cols = ws.as_cols + v * d.N1;
            const double* aff = ws.aff + (size_t)v * MAXT * MAXP;
            int row, col;
            const int np = lsap_solve_wave(nT, m, aff, MAXP, -1.0, rows, cols, row, col);
            if (np < 0 && (tid & 63) == 0) atomicOr(&st.hdr[2], ST_LSAP_INFEASIBLE);
            if ((tid & 63) < np && aff[row * MAXP + col] > 0.0) {
                ws.match_det[row * C + v] = col;
                ws.taken[v * MAXP + col] = 1;
            }
        }
    }
    __syncthreads();
#ifdef PAM_FINE_STAMPS
    if (tid == 0) out_d[13] = now_s();
#endif

    // ---- P3: add_pose (:155-160,289-298), unmatched lists + confidence filter (:56-61,163-167) ----------------
    for (int i = tid; i < nT; i += NT) {
        const int s = st.order[i];
        for (int v = 0; v < C; ++v) {
            const int k = ws.match_det[i * C + v];
            if (k < 0) continue;
            st.already[s] = 1;
            if (st.p2d_time[s * C + v] == T_NONE) { st.p2d_order[s * C + st.p2d_n[s]] = v; st.p2d_n[s] += 1; }
            st.p2d_time[s * C + v] = frame;
            st.cur_det[s * C + v] = k;
        }
    }
    for (int it = tid; it < nT * C * J3; it += NT) {
        const int i = it / (C * J3), r = it % (C * J3), v = r / J3, e = r % J3;
        const int k = ws.match_det[i * C + v];
        if (k >= 0) st.p2d_pose[((size_t)st.order[i] * C + v) * J3 + e] = DET(v, k)[e];
    }
    for (int v = tid; v < C; v += NT) {
        int n = 0;
        for (int k = 0; k < NDET(v); ++k)
            if (!ws.taken[v * MAXP + k] && believe(DET(v, k)) > prm.conf_threshold) ws.um_idx[v * MAXP + n++] = k;
        ws.um_n[v] = n;
    }
    __syncthreads();
    if (tid == 0) out_d[1] = now_s();

    // ---- P4a: views offered to each track (:310-325) and constant-velocity prediction (:341) ------------------
    for (int i = tid; i < nT; i += NT) {
        const int s = st.order[i];
        int n = 0;
        if (st.already[s])
            for (int k = 0; k < st.p2d_n[s]; ++k) {
                const int cid = st.p2d_order[s * C + k];
                const int T = frame - st.p2d_time[s * C + cid];
                if (T <= 3) { ws.sel_cid[i * C + n] = cid; ws.sel_T[i * C + n] = T; ++n; }
            }
        ws.sel_n[i] = (st.already[s] && n >= 2) ? n : 0;
    }
    for (int it = tid; it < nT * J * C; it += NT) ws.conf[it] = 0u;
    for (int it = tid; it < nT * J3; it += NT) {
        const int i = it / J3, e = it % J3, s = st.order[i];
        const int newest = ring_newest(st, s, HCAP);
        const float step = st.vel[s * J3 + e] * (float)(frame - st.hist_time[s * HCAP + newest]);   // float32 product
        ws.pred[i * J3 + e] = st.hist[((size_t)s * HCAP + newest) * J3 + e] + (double)step;
    }
    __syncthreads();

    if (tid == 0) out_d[4] = now_s();
    }                                                    // PART <= 1
    if (PART == 1) {                                     // hand over: hot scratch and integer state back to global memory
        if (A.hot_in_lds) {
            const char* st_lds = hot_lds + hot_bytes(d);
            for (size_t o = (size_t)threadIdx.x * 4; o < hot_bytes(d); o += (size_t)blockDim.x * 4) *(int*)(ws_glob + o) = *(const int*)(hot_lds + o);
            for (size_t o = (size_t)threadIdx.x * 4; o < st_ints; o += (size_t)blockDim.x * 4) *(int*)(st_glob + o) = *(const int*)(st_lds + o);
        }
        if (tid == 0) out_d[15] = now_s();               // split step: end of launch 1 / [12], [13] launch 2's first workgroup / [14] start of launch 3
        return;
    }
    if (PART == 2 && blockIdx.x == 0 && tid == 0) out_d[12] = now_s();
    if (PART == 3 && tid == 0) out_d[14] = now_s();
    // ---- P4b: per-joint conflict sets of the part-aware filter (matching.py:115-151, IterativeTracker.py:345-346): one
    //           lane per (track, joint, view pair r < c), bits OR-ed into the row masks; back-projection ray distances
    //           (matching.py:254-270) one lane per (track, joint, view) ---------------------------------------------------
    int maxV = 0;
    for (int i = 0; i < nT; ++i) maxV = max(maxV, ws.sel_n[i]);
    if (PART != 3) {                                     // (launch 3 of the split step finds the conflict sets and ray distances done)
        const int npair = maxV * (maxV - 1) / 2;
        // joints fastest: the 17 lanes of one (track, view pair) share both fundamental matrices and read consecutive joints
        for (int it = it0; it < nT * npair * J; it += itS) {
            const int i = it / (npair * J), r2 = it % (npair * J), pq = r2 / J, j = r2 % J;
            const int V = ws.sel_n[i];
            // unrank pq -> (r, c), r < c < maxV (row-major over the strict upper triangle), closed form
            const double disc = (2.0 * maxV - 1.0) * (2.0 * maxV - 1.0) - 8.0 * (double)pq;
            int r = (int)((2.0 * maxV - 1.0 - sqrt(disc)) * 0.5);
            while (r > 0 && r * (2 * maxV - r - 1) / 2 > pq) --r;
            while ((r + 1) * (2 * maxV - r - 2) / 2 <= pq) ++r;
            const int c = r + 1 + (pq - r * (2 * maxV - r - 1) / 2);
            if (c >= V) continue;
            const int s = st.order[i];
            const int cr = ws.sel_cid[i * C + r], cc = ws.sel_cid[i * C + c];
            const double dsym = epi_sym(cs, cr, st.p2d_pose + ((size_t)s * C + cr) * J3 + j * 3,
                                        cc, st.p2d_pose + ((size_t)s * C + cc) * J3 + j * 3);
            if (1.0 - dsym / prm.joint_threshold < 0.0) atomicOr(&ws.conf[((size_t)i * J + j) * C + r], 1u << c);
        }
        for (int it = it0; it < nT * J * C; it += itS) {
            const int i = it / (J * C), r2 = it % (J * C), j = r2 / C, r = r2 % C;
            if (r >= ws.sel_n[i]) continue;
            const int s = st.order[i], cr = ws.sel_cid[i * C + r];
            const double* pr = st.p2d_pose + ((size_t)s * C + cr) * J3 + j * 3;
            ws.rayd[((size_t)i * J + j) * C + r] = ray_point_dist(cs.RKINV + cr * 9, cs.pos + cr * 3, pr[1], pr[0], ws.pred + i * J3 + j * 3);
        }
    }
    if (PART == 2) {
        if (blockIdx.x == 0 && tid == 0) out_d[13] = now_s();
        return;
    }
    __syncthreads();

    if (tid == 0) out_d[5] = now_s();
    // ---- P4c: greedy filter (matching.py:243-285) + weighted DLT (construction.py:89-114) per (track, joint); tracks that
    //           see many views split each joint's row folding over 4 lanes and merge the triangular factors ------------
    const int nsplit = maxV > 8 ? DLT_SPLIT : 1;
    for (int it = tid; it < nT * J * nsplit; it += NT) {
        const int ij = it / nsplit, q = it % nsplit, i = ij / J, j = ij % J;
        const int V = ws.sel_n[i];
        if (V == 0) continue;
        const int s = st.order[i];
        uint32_t km;
        if (nsplit == 1 || q == 0) {
            km = greedy_keep_update(V, ws.conf + ((size_t)i * J + j) * C, ws.rayd + ((size_t)i * J + j) * C);
            ws.keep[i * J + j] = km; ws.nview[i * J + j] = __popc(km);
        }
        if (nsplit == 1) {
            double X[3];
            if (__popc(km) >= 2) {
                const int* scid = ws.sel_cid + i * C;
                dlt_joint(cs, V, scid, ws.sel_T + i * C, prm.w_lambda_t, prm.lambda_t, km,
                          [&](int v) { return st.p2d_pose + ((size_t)s * C + scid[v]) * J3 + j * 3; }, X);
            } else {
                X[0] = ws.pred[i * J3 + j * 3]; X[1] = ws.pred[i * J3 + j * 3 + 1]; X[2] = ws.pred[i * J3 + j * 3 + 2];
            }
            ws.raw3d[i * J3 + j * 3] = X[0]; ws.raw3d[i * J3 + j * 3 + 1] = X[1]; ws.raw3d[i * J3 + j * 3 + 2] = X[2];
        }
    }
    if (nsplit > 1) {
        __syncthreads();
        for (int it = tid; it < nT * J * nsplit; it += NT) {
            const int ij = it / nsplit, q = it % nsplit, i = ij / J, j = ij % J;
            const int V = ws.sel_n[i];
            if (V == 0) continue;
            const int s = st.order[i];
            const int* scid = ws.sel_cid + i * C;
            dlt_joint_part(cs, V, q, scid, ws.sel_T + i * C, prm.w_lambda_t, prm.lambda_t, ws.keep[i * J + j],
                           [&](int v) { return st.p2d_pose + ((size_t)s * C + scid[v]) * J3 + j * 3; }, ws.rpart + (size_t)ij * DLT_SPLIT * DLT_PACK);
        }
        __syncthreads();
        for (int it = tid; it < nT * J; it += NT) {
            const int i = it / J, j = it % J;
            if (ws.sel_n[i] == 0) continue;
            double X[3];
            if (ws.nview[i * J + j] >= 2) {
                dlt_joint_merge(ws.rpart + (size_t)it * DLT_SPLIT * DLT_PACK, X);
            } else {
                X[0] = ws.pred[i * J3 + j * 3]; X[1] = ws.pred[i * J3 + j * 3 + 1]; X[2] = ws.pred[i * J3 + j * 3 + 2];
            }
            ws.raw3d[i * J3 + j * 3] = X[0]; ws.raw3d[i * J3 + j * 3 + 1] = X[1]; ws.raw3d[i * J3 + j * 3 + 2] = X[2];
        }
    }
    __syncthreads();

    if (tid == 0) out_d[6] = now_s();
    // ---- P4d: success test (:369) ------------------------------------------------------------------------------
    for (int i = tid; i < nT; i += NT) {
        int okv = 0;
        if (ws.sel_n[i] > 0) {
            int fails = 0;
            for (int j = 0; j < J; ++j) fails += (ws.nview[i * J + j] < 2);
            okv = !(3 * fails > J);
        }
        ws.ok[i] = okv;
    }
    __syncthreads();

    if (tid == 0) out_d[7] = now_s();
    // ---- P4e: temporal smoothing into the next ring entry (:371-383) -------------------------------------------
    for (int it = tid; it < nT * J3; it += NT) {
        const int i = it / J3, e = it % J3;
        if (!ws.ok[i]) continue;
        const int s = st.order[i], j = e / 3;
        const int head = st.h_head[s], len = st.h_len[s];
        const bool arm = (j == 9 || j == 10);
        const double* hs = st.hist + (size_t)s * HCAP * J3;
        const double raw = ws.raw3d[i * J3 + e];
        const double val = smooth_last(len + 1, arm ? prm.n_taps_arm : prm.n_taps_body, arm ? prm.taps_arm : prm.taps_body,
                                       [&](int q) { return q < len ? hs[((head + q) % HCAP) * J3 + e] : raw; });
        st.hist[((size_t)s * HCAP + (head + len) % HCAP) * J3 + e] = val;
    }
    __syncthreads();
    if (tid == 0) out_d[8] = now_s();
    // ---- P4f: append + prune history (:330-332) ---------------------------------------------------------------
    for (int i = tid; i < nT; i += NT) {
        if (!ws.ok[i]) continue;
        const int s = st.order[i];
        int head = st.h_head[s], len = st.h_len[s];
        st.hist_time[s * HCAP + (head + len) % HCAP] = frame;
        ++len;
        for (int j = 0; j < J; ++j) st.jv_count[s * J + j] = ws.nview[i * J + j];
        st.jv_V[s] = ws.sel_n[i];
        if (frame - st.hist_time[s * HCAP + head] > prm.max_age) { head = (head + 1) % HCAP; --len; }
        st.h_head[s] = head; st.h_len[s] = len;
    }
    __syncthreads();
    if (tid == 0) out_d[9] = now_s();
    // ---- P4g: float32 velocity (:385-395) and life cycle (:253-274) -------------------------------------------
    for (int it = tid; it < nT * J3; it += NT) {
        const int i = it / J3, e = it % J3;
        if (!ws.ok[i]) continue;
        const int s = st.order[i];
        const int head = st.h_head[s], len = st.h_len[s];
        if (len < 2) continue;
        const double* hs = st.hist + (size_t)s * HCAP * J3;
        st.vel[s * J3 + e] = velocity_f32(len, [&](int q) { return hs[((head + q) % HCAP) * J3 + e]; });
    }
    for (int i = tid; i < nT; i += NT) {
        const int s = st.order[i];
        if (ws.ok[i]) {
            st.hits[s] += 1; st.tsu[s] = 0;
            if (st.state[s] == TENTATIVE && st.hits[s] >= prm.n_init) st.state[s] = CONFIRMED;
        } else {
            if (st.state[s] == TENTATIVE && !st.already[s]) st.state[s] = DELETED;
            else if (st.tsu[s] >= prm.max_age) st.state[s] = DELETED;
        }
    }
    __syncthreads();
    if (tid == 0) out_d[2] = now_s();

    // ---- P5: init_target_GD (:52-113): greedy cross-view hypotheses from the unmatched detections ------------
    if (tid == 0) ws.misc[0] = 0;
    __syncthreads();
    // (steady state: every detection was matched -- no hypothesis can form, and the block below is 2 C + 5 workgroup barriers: 62 on the
    //  31-camera rig, 9 of its 143 us)
    int um_total = 0;
    for (int v = 0; v < C; ++v) um_total += ws.um_n[v];
    if (C >= 2 && um_total > 0) {
        if (tid == 0) {
            int nh = 0;
            for (int k = 0; k < ws.um_n[0]; ++k) {
                if (nh >= MAXH) { atomicOr(&st.hdr[2], ST_HYP_OVERFLOW); break; }
                ws.hyp_size[nh] = 1; ws.hyp_view[nh * C] = 0; ws.hyp_det[nh * C] = ws.um_idx[k]; ++nh;
            }
            ws.misc[0] = nh;
        }
        __syncthreads();
        for (int v = 1; v < C; ++v) {
            const int nh = ws.misc[0], nd = ws.um_n[v];
            if (nh > 0 && nd > 0) {
                for (int it = tid; it < nh * nd; it += NT) {   // Hypothesis.calculate_cost (hypothesis.py:53-68)
                    const int h = it / nd, k = it % nd;
                    const double* po = DET(v, ws.um_idx[v * MAXP + k]);
                    const double bel = believe(po);
                    double total = 0.0; int veto = 0;
                    const int sz = ws.hyp_size[h];
                    for (int q = 0; q < sz; ++q) {
                        const int cm = ws.hyp_view[h * C + q];
                        const double p = hyp_member_cost(cs, cm, DET(cm, ws.hyp_det[h * C + q]), v, po, prm.epi_threshold);
                        total += p;
                        if (p > 1.0 && bel > 0.5) veto = 1;
                    }
                    ws.hc_cost[h * MAXP + k] = total / (double)sz;
                    ws.hc_veto[h * MAXP + k] = (unsigned char)veto;
                }
            }
            __syncthreads();
            if (tid == 0 && nd > 0) {
                int np = 0;
                if (nh > 0) {
                    LsapScratch sc = lsap_carve(ws.lsap2, d.N2);
                    np = lsap_solve(nh, nd, ws.hc_cost, MAXP, 1.0, sc, ws.l2_rows, ws.l2_cols);
                    if (np < 0) { atomicOr(&st.hdr[2], ST_LSAP_INFEASIBLE); np = 0; }
                }
                uint32_t handled = 0;
                int nh2 = nh;
                for (int q = 0; q < np; ++q) {
                    const int h = ws.l2_rows[q], k = ws.l2_cols[q];
                    handled |= 1u << k;
                    if (ws.hc_veto[h * MAXP + k]) {
                        if (nh2 >= MAXH) { atomicOr(&st.hdr[2], ST_HYP_OVERFLOW); continue; }
                        ws.hyp_size[nh2] = 1; ws.hyp_view[nh2 * C] = v; ws.hyp_det[nh2 * C] = ws.um_idx[v * MAXP + k]; ++nh2;
                    } else {
                        const int sz = ws.hyp_size[h];
                        ws.hyp_view[h * C + sz] = v; ws.hyp_det[h * C + sz] = ws.um_idx[v * MAXP + k]; ws.hyp_size[h] = sz + 1;
                    }
                }
                for (int k = 0; k < nd; ++k)
                    if (!((handled >> k) & 1u)) {
                        if (nh2 >= MAXH) { atomicOr(&st.hdr[2], ST_HYP_OVERFLOW); continue; }
                        ws.hyp_size[nh2] = 1; ws.hyp_view[nh2 * C] = v; ws.hyp_det[nh2 * C] = ws.um_idx[v * MAXP + k]; ++nh2;
                    }
                ws.misc[0] = nh2;
            }
            __syncthreads();
        }
        // -- Hypothesis.get_3dpose_jf (hypothesis.py:23-44): float32 loop-form distances, init-mode filter, DLT ----
        const int nh = ws.misc[0];
        const float thr32 = (float)prm.init_threshold;
        for (int it = tid; it < nh * J * C; it += NT) {
            const int h = it / (J * C), r2 = it % (J * C), j = r2 / C, r = r2 % C;
            const int V = ws.hyp_size[h];
            if (V < 2 || r >= V) continue;
            const int* hv = ws.hyp_view + h * C; const int* hd = ws.hyp_det + h * C;
            uint32_t bits = 0;
            const float sum = np_sum_f32(V, [&](int c) -> float {
                if (c == r) return 1.0f - 0.0f / thr32;
                const int lo = c < r ? c : r, hi = c < r ? r : c;
                const float d32 = epi_sym_init(cs, hv[lo], DET(hv[lo], hd[lo]) + j * 3, hv[hi], DET(hv[hi], hd[hi]) + j * 3);
                const float a = 1.0f - d32 / thr32;
                if (c > r && a < 0.0f) bits |= 1u << c;
                return a;
            });
            ws.h_conf[((size_t)h * J + j) * C + r] = bits;
            ws.h_sum[((size_t)h * J + j) * C + r] = sum;
        }
        __syncthreads();
        for (int it = tid; it < nh * J; it += NT) {
            const int h = it / J, j = it % J;
            const int V = ws.hyp_size[h];
            if (V < 2) continue;
            const uint32_t km = greedy_keep_init(V, ws.h_conf + ((size_t)h * J + j) * C, ws.h_sum + ((size_t)h * J + j) * C);
            ws.h_keep[h * J + j] = km;
            if (__popc(km) >= 2) {
                const int* hv = ws.hyp_view + h * C; const int* hd = ws.hyp_det + h * C;
                double X[3];   // ages are all 0 at initialisation (hypothesis.py:24-27)
                dlt_joint(cs, V, hv, g_zeroT, prm.w_lambda_t, prm.lambda_t, km,
                          [&](int v) { return DET(hv[v], hd[v]) + j * 3; }, X);
                ws.h_pose[h * J3 + j * 3] = X[0]; ws.h_pose[h * J3 + j * 3 + 1] = X[1]; ws.h_pose[h * J3 + j * 3 + 2] = X[2];
            }
        }
        __syncthreads();
        if (tid == 0) {   // spawn tracks in hypothesis order (:102-113)
            int n = st.hdr[0];
            unsigned long long used = ((unsigned long long)(unsigned)st.hdr[4] << 32) | (unsigned)st.hdr[3];
            for (int h = 0; h < nh; ++h) {
                ws.h_slot[h] = -1;
                const int V = ws.hyp_size[h];
                if (V < 2) continue;
                bool good = true;
                for (int j = 0; j < J; ++j) if (__popc(ws.h_keep[h * J + j]) < 2) { good = false; break; }
                if (!good) continue;
                int s = -1;
                for (int q = 0; q < MAXT; ++q) if (!((used >> q) & 1ull)) { s = q; break; }
                if (s < 0) { atomicOr(&st.hdr[2], ST_TRACK_OVERFLOW); continue; }
                used |= 1ull << s;
                st.track_id[s] = st.hdr[1]; st.hdr[1] += 1;
                st.hits[s] = 1; st.age[s] = 1; st.tsu[s] = 0; st.already[s] = 0; st.state[s] = TENTATIVE;
                st.p2d_n[s] = V; st.h_head[s] = 0; st.h_len[s] = 1; st.hist_time[s * HCAP] = frame; st.jv_V[s] = V;
                for (int c = 0; c < C; ++c) { st.p2d_time[s * C + c] = T_NONE; st.cur_det[s * C + c] = -1; }
                for (int q = 0; q < V; ++q) {
                    const int cid = ws.hyp_view[h * C + q];
                    st.p2d_order[s * C + q] = cid; st.p2d_time[s * C + cid] = frame; st.cur_det[s * C + cid] = ws.hyp_det[h * C + q];
                }
                for (int j = 0; j < J; ++j) st.jv_count[s * J + j] = __popc(ws.h_keep[h * J + j]);
                st.order[n++] = s;
                ws.h_slot[h] = s;
            }
            st.hdr[0] = n; st.hdr[3] = (int)(unsigned)(used & 0xffffffffull); st.hdr[4] = (int)(unsigned)(used >> 32);
        }
        __syncthreads();
        for (int it = tid; it < nh * (C + 1) * J3; it += NT) {   // pose copies of the new tracks
            const int h = it / ((C + 1) * J3), r = it % ((C + 1) * J3), q = r / J3, e = r % J3;
            const int s = ws.h_slot[h];
            if (s < 0) continue;
            const int V = ws.hyp_size[h];
            if (q < V) {
                const int cid = ws.hyp_view[h * C + q];
                st.p2d_pose[((size_t)s * C + cid) * J3 + e] = DET(cid, ws.hyp_det[h * C + q])[e];
            } else if (q == C) {
                st.hist[(size_t)s * HCAP * J3 + e] = ws.h_pose[h * J3 + e];
                st.vel[s * J3 + e] = 0.0f;
            }
        }
        __syncthreads();
    }
    if (tid == 0) out_d[3] = now_s();

    if (tid == 0) out_d[10] = now_s();
    // ---- P6: drop deleted tracks, keep list order (:178) ------------------------------------------------------
    if (tid == 0) {
        const int n = st.hdr[0];
        unsigned long long used = ((unsigned long long)(unsigned)st.hdr[4] << 32) | (unsigned)st.hdr[3];
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int s = st.order[i];
            if (st.state[s] == DELETED) used &= ~(1ull << s); else st.order[m++] = s;
        }
        st.hdr[0] = m; st.hdr[3] = (int)(unsigned)(used & 0xffffffffull); st.hdr[4] = (int)(unsigned)(used >> 32);
        // status word: bits 0-15 = this frame, bits 16-31 = OR over every frame since pam_create / pam_reset (a host that
        // only decodes the last record of a run still sees an overflow raised in any earlier frame)
        st.hdr[5] |= st.hdr[2];
        st.hdr[6] = 0;                                  // a frame was applied: the run of void frames (input guard above), if any, is over
        out_i[0] = m; out_i[1] = (st.hdr[2] & 0xffff) | (st.hdr[5] << 16); out_i[2] = frame; out_i[3] = ws.misc[0];
    }
    __syncthreads();

    // ---- P7: output record (ivclabpose.py:259-287 + state for parity tests) -----------------------------------
    const int nOut = st.hdr[0];
    const PamOutLayout ol = A.ol;
    for (int i = tid; i < nOut; i += NT) {
        const int s = st.order[i];
        int* o = out_i + ol.hdr_words + i * ol.trk_words;
        const int newest = ring_newest(st, s, HCAP);
        o[0] = st.track_id[s]; o[1] = st.state[s]; o[2] = st.hits[s]; o[3] = st.age[s]; o[4] = st.tsu[s];
        o[5] = (st.tsu[s] == 0 && st.state[s] == CONFIRMED) ? 1 : 0;
        o[6] = st.p2d_n[s]; o[7] = st.jv_V[s]; o[8] = st.h_len[s]; o[9] = st.hist_time[s * HCAP + newest];
    }
    for (int it = tid; it < nOut * (C + J); it += NT) {    // the per-view and per-joint fields: a lane per (track, field), not a lane per track
        const int i = it / (C + J), c = it % (C + J), s = st.order[i];
        int* o = out_i + ol.hdr_words + i * ol.trk_words;
        if (c < C) {
            o[ol.off_order + c] = (c < st.p2d_n[s]) ? st.p2d_order[s * C + c] : -1;
            o[ol.off_matched + c] = st.cur_det[s * C + c];
            o[ol.off_time2d + c] = st.p2d_time[s * C + c];
        } else {
            o[ol.off_nviews + (c - C)] = st.jv_count[s * J + (c - C)];
        }
    }
    for (int it = tid; it < nOut * J3; it += NT) {
        const int i = it / J3, e = it % J3, s = st.order[i];
        const int newest = ring_newest(st, s, HCAP);
        double* o = out_d + ol.dbl_hdr_words + (size_t)i * ol.dbl_trk_words;
        o[e] = st.hist[((size_t)s * HCAP + newest) * J3 + e];
        o[J3 + e] = (double)st.vel[s * J3 + e];
    }
    if (tid == 0) out_d[11] = now_s();
    if (A.hot_in_lds) {                                                 // integer scene state back to HBM
        __syncthreads();
        const char* st_lds = hot_lds + hot_bytes(d);
        for (size_t o = (size_t)threadIdx.x * 4; o < st_ints; o += (size_t)blockDim.x * 4) *(int*)(st_glob + o) = *(const int*)(st_lds + o);
    }
#undef DET
#undef NDET
}

// =====================================================================================================================
// The parity kernel of the assignment solver (pam_op_lsap).  It stays in this file: lsap_solve_wave is a plain inline function, and while
// k_frame is its only caller in a translation unit the device compiler narrows it to k_frame's argument ranges before inlining it, which
// changes k_frame's registers and schedule.  A second caller with free arguments keeps k_frame's code what it was (tools/device_code_diff.py).
// =====================================================================================================================
__global__ void k_op_lsap(int nr, int nc, const double* cost, char* scratch, int N, int* rows, int* cols, int* np) {
    // one wave: the solver the frame kernel runs per view (N <= 64); beyond that the single-lane form the hypothesis step uses
    if (N <= 64) {
        int row, col;
        const int n = lsap_solve_wave(nr, nc, cost, nc, 1.0, rows, cols, row, col);
        if (threadIdx.x == 0) *np = n;
    } else if (threadIdx.x == 0) {
        LsapScratch sc = lsap_carve(scratch, N);
        *np = lsap_solve(nr, nc, cost, nc, 1.0, sc, rows, cols);
    }
}

// How the step runs on a handle: one helper for launch_frame and pam_frame_plan
struct FramePlan { int block, launches, hot_in_lds; size_t hot; };
static FramePlan frame_plan(const PamHandle* h) {
    FramePlan p;
    // hot scratch + integer state: kept in LDS for the frame when they fit
    p.hot = hot_bytes(h->d) + ((state_int_bytes(h->d) + 15) & ~(size_t)15);
    p.hot_in_lds = p.hot <= 128 * 1024 ? 1 : 0;
    // one workgroup per scene; many-camera rigs have ~10^4-10^5 independent (track, view pair, joint) items per frame, so
    // they get the largest workgroup (16 waves hide the L2 latency of the pose / fundamental-matrix reads)
    p.block = h->d.C > 8 ? 1024 : BLOCK;
    // wide rigs, one scene: three launches, the conflict sets of P4b over the whole chip (PAM_FRAME_SPLIT=0: the single launch, for A/B runs)
    static const int split_ok = getenv("PAM_FRAME_SPLIT") ? atoi(getenv("PAM_FRAME_SPLIT")) : 1;
    p.launches = (p.block == 1024 && h->d.S == 1 && split_ok) ? 3 : 1;
    return p;
}

extern "C" int pam_frame_plan(const PamHandle* h, int32_t* block, int32_t* launches, int32_t* hot_in_lds) {
    if (!h || !block || !launches || !hot_in_lds) return PAM_E_ARG;
    const FramePlan p = frame_plan(h);
    *block = p.block; *launches = p.launches; *hot_in_lds = p.hot_in_lds;
    return PAM_OK;
}

static int launch_frame(PamHandle* h, hipStream_t s, int frame_id, const int* d_ndet, const double* d_det, const int* d_view_row = nullptr) {
    if (!h->cams_set) { h->err = "pam_set_cameras has not been called"; return PAM_E_STATE; }
    FrameArgs A;
    A.d = h->d; A.cs = camset(h); A.prm = h->d_prm;
    A.state = h->d_state; A.state_stride = h->state_stride; A.ws = h->d_ws; A.ws_stride = h->ws_stride;
    A.guard = h->d_guard;
    A.n_det = d_ndet; A.det = d_det; A.view_row = d_view_row; A.out_i = h->d_out_i; A.out_d = h->d_out_d; A.ol = h->ol; A.frame_id = frame_id;
    const FramePlan plan = frame_plan(h);
    const size_t hot = plan.hot;
    A.hot_in_lds = plan.hot_in_lds;
    const int block = plan.block;
    // each workgroup size is its own instantiation with its own __launch_bounds__: under a shared bound of 1024 the 256-thread
    // form was held to 128 VGPRs (occupancy 4) and spilled 211 SGPRs
#ifdef PAM_DIAG
    static const int dblock = getenv("PAM_FRAME_BLOCK") ? atoi(getenv("PAM_FRAME_BLOCK")) : 0;
    static const int dlds = getenv("PAM_FRAME_LDS") ? atoi(getenv("PAM_FRAME_LDS")) : 1;
    if (!dlds) A.hot_in_lds = 0;
    if (getenv("PAM_FRAME_VERBOSE")) fprintf(stderr, "k_frame: hot bytes %zu, block %d\n", hot, dblock ? dblock : block);
    if (dblock == 64) { hipLaunchKernelGGL(k_frame<64>, dim3(h->d.S), dim3(64), A.hot_in_lds ? hot : 0, s, A); HIPCHK(h, hipGetLastError()); return PAM_OK; }
    if (dblock == 128) { hipLaunchKernelGGL(k_frame<128>, dim3(h->d.S), dim3(128), A.hot_in_lds ? hot : 0, s, A); HIPCHK(h, hipGetLastError()); return PAM_OK; }
#endif
    if (plan.launches == 3) {
        // launches 1 and 3 keep the hot scratch and the integer state in LDS (the serial LSAP walks live there) and hand them over through
        // their home in global memory; launch 2 works on the global copy
        const int in_lds = A.hot_in_lds;
        hipLaunchKernelGGL((k_frame<1024, 1>), dim3(1), dim3(1024), in_lds ? hot : 0, s, A);
        A.hot_in_lds = 0;
        hipLaunchKernelGGL((k_frame<256, 2>), dim3(256), dim3(256), 0, s, A);
        A.hot_in_lds = in_lds;
        hipLaunchKernelGGL((k_frame<1024, 3>), dim3(1), dim3(1024), in_lds ? hot : 0, s, A);
    }
    else if (block == 1024) hipLaunchKernelGGL(k_frame<1024>, dim3(h->d.S), dim3(1024), A.hot_in_lds ? hot : 0, s, A);
    else hipLaunchKernelGGL(k_frame<BLOCK>, dim3(h->d.S), dim3(BLOCK), A.hot_in_lds ? hot : 0, s, A);
    HIPCHK(h, hipGetLastError());
    return PAM_OK;
}

extern "C" int pam_frame_dev(PamHandle* h, void* stream, int frame_id, const int32_t* dev_n_det, const double* dev_det) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, dev_n_det && dev_det, "null device buffer");
    return launch_frame(h, (hipStream_t)stream, frame_id, dev_n_det, dev_det);
}

// The frame on view-sharded input: dev_records = the buffer pam_allgather_keypoints (or any all-gather of the ranks' send buffers)
// filled, dev_view_row[v] = which of its records holds view v.  The kernel reads the records in place: no unpack kernel, no copies.
extern "C" int pam_frame_dev_views(PamHandle* h, void* stream, int frame_id, const double* dev_records, const int32_t* dev_view_row) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, dev_records && dev_view_row, "null device buffer");
    ARGCHK(h, h->d.S == 1, "view-sharded input is one scene per handle");
    return launch_frame(h, (hipStream_t)stream, frame_id, nullptr, dev_records, dev_view_row);
}

extern "C" int pam_frame(PamHandle* h, int frame_id, const int32_t* n_det, const double* det, int32_t* out_i, double* out_d) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, n_det && det, "null input");
    const Dims& d = h->d;
    for (int i = 0; i < d.S * d.C; ++i) ARGCHK(h, n_det[i] >= 0 && n_det[i] <= d.MAXP, "n_det exceeds max_dets");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d_ndet, n_det, sizeof(int) * d.S * d.C, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_det, det, sizeof(double) * (size_t)d.S * d.C * d.MAXP * J3, hipMemcpyHostToDevice, h->stream));
    int rc = launch_frame(h, h->stream, frame_id, h->d_ndet, h->d_det);
    if (rc) return rc;
    if (out_i) HIPCHK(h, hipMemcpyAsync(out_i, h->d_out_i, out_int_bytes(h), hipMemcpyDeviceToHost, h->stream));
    if (out_d) HIPCHK(h, hipMemcpyAsync(out_d, h->d_out_d, out_dbl_bytes(h), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (out_i)
        for (int s = 0; s < d.S; ++s)
            if (out_i[(size_t)s * h->ol.int_words + 1] & (ST_TRACK_OVERFLOW | ST_HYP_OVERFLOW)) {
                h->err = "scene ran out of track or hypothesis slots (raise max_tracks / max_hyps)";
                return PAM_E_OVERFLOW;
            }
    return PAM_OK;
}

extern "C" int pam_op_lsap(PamHandle* h, int nr, int nc, const double* cost, int32_t* rows, int32_t* cols, int32_t* n_pairs) {
    if (!h) return PAM_E_ARG;
    OpStage S(h, __func__);
    ARGCHK(h, nr >= 0 && nc >= 0 && nr <= 1024 && nc <= 1024, "bad shape");
    if (nr == 0 || nc == 0) { *n_pairs = 0; return PAM_OK; }
    const int N = nr > nc ? nr : nc;
    const double* c = S.in(cost, (size_t)nr * nc);
    char* sc = S.out<char>(lsap_scratch_bytes(N) + 8);
    int* r = S.out<int>(N); int* cc = S.out<int>(N); int* np = S.out<int>(1);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_lsap, dim3(1), dim3(64), 0, 0, nr, nc, c, (char*)(((uintptr_t)sc + 7) & ~(uintptr_t)7), N, r, cc, np);
    int rc = S.done(); if (rc) return rc;
    S.back(n_pairs, np, 1);                                  // the copy-back sizes depend on it
    if (*n_pairs < 0) { h->err = "infeasible cost matrix"; return PAM_E_ARG; }
    S.back(rows, r, *n_pairs); S.back(cols, cc, *n_pairs);
    return S.status();
}

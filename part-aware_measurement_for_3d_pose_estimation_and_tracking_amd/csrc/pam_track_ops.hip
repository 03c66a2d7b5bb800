// libpam_hip.so, tracker part: the per-operator kernels of the parity tests and their entry points (pam_op_*).  gfx950 only.
#include "pam_tracker.hpp"

// =====================================================================================================================
// Per-operator kernels (parity tests): thin wrappers over the same device functions.
// =====================================================================================================================
__global__ void k_op_project(CamSet cs, int cid, int n, const double* poses, double* out) {
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < n * J; it += gridDim.x * blockDim.x) {
        double u, v;
        project_point(cs.P + cid * 12, poses[it * 3], poses[it * 3 + 1], poses[it * 3 + 2], u, v);
        out[it * 2] = v; out[it * 2 + 1] = u;
    }
}
__global__ void k_op_affinity(CamSet cs, const PamParams* prm, int cid, int n, int m, const double* tp, const int* dt,
                              const double* dets, double* aff) {
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < n * m; it += gridDim.x * blockDim.x) {
        const int i = it / m, k = it % m, t = dt[i];
        const double e = (t >= 0 && t < PAM_EXP_TABLE) ? prm->exp_lambda_a[t] : exp(prm->lambda_a * (double)t);
        aff[it] = track_det_affinity(cs.P + cid * 12, tp + (size_t)i * J3, dets + (size_t)k * J3, prm->alpha2d * (double)t, e,
                                     prm->count_gate);
    }
}
__global__ void k_op_epi_dist(CamSet cs, int V, const int* cids, const double* pm, double* dist) {
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < V * V * J; it += gridDim.x * blockDim.x) {
        const int a = it / (V * J), r = it % (V * J), b = r / J, j = r % J;
        dist[it] = epi_sym(cs, cids[a], pm + ((size_t)a * J + j) * 3, cids[b], pm + ((size_t)b * J + j) * 3);
    }
}
__global__ void k_op_epi_pair(CamSet cs, int c1, const double* p1, int c2, const double* p2, double* out) {
    const int j = threadIdx.x;
    if (j < J) {
        double d1, d2;
        epi_pair_cv(cs.F + ((size_t)c1 * cs.C + c2) * 9, p1[j * 3 + 1], p1[j * 3], p2[j * 3 + 1], p2[j * 3], d1, d2);
        out[j * 2] = d1; out[j * 2 + 1] = d2;
    }
}
__global__ void k_op_epi_dist_init(CamSet cs, int V, const int* cids, const double* pm, float* dist) {
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < V * V * J; it += gridDim.x * blockDim.x) {
        const int a = it / (V * J), r = it % (V * J), b = r / J, j = r % J;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        dist[it] = (a == b) ? 0.0f : epi_sym_init(cs, cids[lo], pm + ((size_t)lo * J + j) * 3, cids[hi], pm + ((size_t)hi * J + j) * 3);
    }
}
__global__ void k_op_greedy(CamSet cs, int mode, int V, const int* cids, const void* aff, const double* pose_j,
                            const double* next_j, uint32_t* conf, double* ray, float* sums, uint32_t* keep) {
    const int r = threadIdx.x;
    if (r < V) {
        uint32_t bits = 0;
        if (mode == 0) {
            const double* a = (const double*)aff;
            for (int c = r + 1; c < V; ++c) if (a[r * V + c] < 0.0) bits |= 1u << c;
            ray[r] = ray_point_dist(cs.RKINV + cids[r] * 9, cs.pos + cids[r] * 3, pose_j[r * 3 + 1], pose_j[r * 3], next_j);
        } else {
            const float* a = (const float*)aff;
            for (int c = r + 1; c < V; ++c) if (a[r * V + c] < 0.0f) bits |= 1u << c;
            sums[r] = np_sum_f32(V, [&](int c) { return a[r * V + c]; });
        }
        conf[r] = bits;
    }
    __syncthreads();
    if (threadIdx.x == 0) *keep = (mode == 0) ? greedy_keep_update(V, conf, ray) : greedy_keep_init(V, conf, sums);
}
__global__ void k_op_dlt(CamSet cs, const PamParams* prm, int V, const int* cids, const int* Ts, const double* pm,
                         const uint32_t* keep, const double* next_pose, double* out) {
    const int j = threadIdx.x;
    if (j < J) {
        double X[3];
        if (__popc(keep[j]) >= 2)
            dlt_joint(cs, V, cids, Ts, prm->w_lambda_t, prm->lambda_t, keep[j],
                      [&](int v) { return pm + ((size_t)v * J + j) * 3; }, X);
        else { X[0] = next_pose[j * 3]; X[1] = next_pose[j * 3 + 1]; X[2] = next_pose[j * 3 + 2]; }
        out[j * 3] = X[0]; out[j * 3 + 1] = X[1]; out[j * 3 + 2] = X[2];
    }
}
// the same joints with the paths of P4c selectable: nsplit 1 = dlt_joint, nsplit DLT_SPLIT = the fold / pack / merge / solve sequence of the
// wide rigs (part: 17 x DLT_SPLIT x DLT_PACK doubles); jacobi_only = the fall-back alone; path[j] = DLT_PATH_* of joint j.  One workgroup.
__global__ void k_op_dlt_paths(CamSet cs, const PamParams* prm, int V, const int* cids, const int* Ts, const double* pm,
                               const uint32_t* keep, const double* next_pose, int nsplit, int jacobi_only, double* part, double* out,
                               int* path) {
    const int tid = threadIdx.x;
    if (nsplit > 1) {
        for (int it = tid; it < J * DLT_SPLIT; it += blockDim.x) {
            const int j = it / DLT_SPLIT, q = it % DLT_SPLIT;
            dlt_joint_part(cs, V, q, cids, Ts, prm->w_lambda_t, prm->lambda_t, keep[j],
                           [&](int v) { return pm + ((size_t)v * J + j) * 3; }, part + (size_t)j * DLT_SPLIT * DLT_PACK);
        }
        __syncthreads();
    }
    const int j = tid;
    if (j < J) {
        double X[3];
        int p = DLT_PATH_COPIED;
        if (__popc(keep[j]) < 2) { X[0] = next_pose[j * 3]; X[1] = next_pose[j * 3 + 1]; X[2] = next_pose[j * 3 + 2]; }
        else if (nsplit > 1) p = dlt_joint_merge(part + (size_t)j * DLT_SPLIT * DLT_PACK, X, jacobi_only != 0);
        else p = dlt_joint(cs, V, cids, Ts, prm->w_lambda_t, prm->lambda_t, keep[j],
                           [&](int v) { return pm + ((size_t)v * J + j) * 3; }, X, jacobi_only != 0);
        out[j * 3] = X[0]; out[j * 3 + 1] = X[1]; out[j * 3 + 2] = X[2];
        path[j] = p;
    }
}
__global__ void k_op_smooth(const PamParams* prm, int L, const double* hist, const double* raw, double* out) {
    const int e = threadIdx.x;
    if (e < J3) {
        const int j = e / 3;
        const bool arm = (j == 9 || j == 10);
        out[e] = smooth_last(L + 1, arm ? prm->n_taps_arm : prm->n_taps_body, arm ? prm->taps_arm : prm->taps_body,
                             [&](int q) { return q < L ? hist[(size_t)q * J3 + e] : raw[e]; });
    }
}
__global__ void k_op_velocity(int L, const double* hist, float* vel) {
    const int e = threadIdx.x;
    if (e < J3) vel[e] = velocity_f32(L, [&](int q) { return hist[(size_t)q * J3 + e]; });
}
__global__ void k_op_hyp_cost(CamSet cs, const PamParams* prm, int n, const int* cids, const double* poses, int o_cid,
                              const double* o_pose, double* cost, int* veto) {
    if (threadIdx.x == 0) {
        const double bel = believe(o_pose);
        double total = 0.0; int vt = 0;
        for (int q = 0; q < n; ++q) {
            const double p = hyp_member_cost(cs, cids[q], poses + (size_t)q * J3, o_cid, o_pose, prm->epi_threshold);
            total += p;
            if (p > 1.0 && bel > 0.5) vt = 1;
        }
        *cost = total / (double)n; *veto = vt;
    }
}

// ---- per-operator entry points: stage to the handle's op buffer (OpStage, pam_tracker.hpp), run, copy back ---------------------
// (pam_op_lsap sits beside k_frame in pam_frame.hip)
#define OP_PROLOG(h) if (!(h)) return PAM_E_ARG; if (!(h)->cams_set) { (h)->err = "pam_set_cameras has not been called"; return PAM_E_STATE; } OpStage S(h, __func__)

extern "C" int pam_op_project(PamHandle* h, int cid, int n, const double* poses3d, double* out_yx) {
    OP_PROLOG(h);
    ARGCHK(h, cid >= 0 && cid < h->d.C && n >= 0, "bad cid / n");
    if (n == 0) return PAM_OK;
    const double* p = S.in(poses3d, (size_t)n * J3); double* o = S.out<double>((size_t)n * J * 2);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_project, dim3((n * J + 255) / 256), dim3(256), 0, 0, camset(h), cid, n, p, o);
    return S.finish(out_yx, o, (size_t)n * J * 2);
}

extern "C" int pam_op_track_affinity(PamHandle* h, int cid, int n, int m, const double* tracks_pose, const int32_t* dt,
                                     const double* dets, double* aff) {
    OP_PROLOG(h);
    ARGCHK(h, cid >= 0 && cid < h->d.C && n > 0 && m > 0, "bad cid / n / m");
    const double* tp = S.in(tracks_pose, (size_t)n * J3); const int* t = S.in(dt, n);
    const double* dd = S.in(dets, (size_t)m * J3); double* o = S.out<double>((size_t)n * m);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_affinity, dim3((n * m + 63) / 64), dim3(64), 0, 0, camset(h), h->d_prm, cid, n, m, tp, t, dd, o);
    return S.finish(aff, o, (size_t)n * m);
}

extern "C" int pam_op_epi_dist(PamHandle* h, int V, const int32_t* cids, const double* pose_mat, double* dist) {
    OP_PROLOG(h);
    ARGCHK(h, V >= 1 && V <= PAM_MAX_VIEWS, "bad V");
    const int* c = S.in(cids, V); const double* pm = S.in(pose_mat, (size_t)V * J3); double* o = S.out<double>((size_t)V * V * J);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_epi_dist, dim3((V * V * J + 255) / 256), dim3(256), 0, 0, camset(h), V, c, pm, o);
    return S.finish(dist, o, (size_t)V * V * J);
}

extern "C" int pam_op_epi_pair(PamHandle* h, int c1, const double* person1, int c2, const double* person2, double* out) {
    OP_PROLOG(h);
    ARGCHK(h, c1 >= 0 && c1 < h->d.C && c2 >= 0 && c2 < h->d.C, "bad camera id");
    const double* p1 = S.in(person1, J3); const double* p2 = S.in(person2, J3); double* o = S.out<double>(J * 2);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_epi_pair, dim3(1), dim3(64), 0, 0, camset(h), c1, p1, c2, p2, o);
    return S.finish(out, o, J * 2);
}

extern "C" int pam_op_epi_dist_init(PamHandle* h, int V, const int32_t* cids, const double* pose_mat, float* dist) {
    OP_PROLOG(h);
    ARGCHK(h, V >= 1 && V <= PAM_MAX_VIEWS, "bad V");
    const int* c = S.in(cids, V); const double* pm = S.in(pose_mat, (size_t)V * J3); float* o = S.out<float>((size_t)V * V * J);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_epi_dist_init, dim3((V * V * J + 255) / 256), dim3(256), 0, 0, camset(h), V, c, pm, o);
    return S.finish(dist, o, (size_t)V * V * J);
}

extern "C" int pam_op_greedy(PamHandle* h, int mode, int V, const int32_t* cids, const void* aff, const double* pose_j,
                             const double* next_pose_j, uint32_t* keep_mask) {
    OP_PROLOG(h);
    ARGCHK(h, V >= 1 && V <= PAM_MAX_VIEWS && (mode == 0 || mode == 1), "bad V / mode");
    const int* c = S.in(cids, V);
    const void* a = (mode == 0) ? (const void*)S.in((const double*)aff, (size_t)V * V) : (const void*)S.in((const float*)aff, (size_t)V * V);
    const double* pj = (mode == 0) ? S.in(pose_j, (size_t)V * 3) : nullptr;
    const double* nj = (mode == 0) ? S.in(next_pose_j, 3) : nullptr;
    uint32_t* conf = S.out<uint32_t>(V); double* ray = S.out<double>(V); float* sums = S.out<float>(V); uint32_t* k = S.out<uint32_t>(1);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_greedy, dim3(1), dim3(64), 0, 0, camset(h), mode, V, c, a, pj, nj, conf, ray, sums, k);
    return S.finish(keep_mask, k, 1);
}

extern "C" int pam_op_dlt(PamHandle* h, int V, const int32_t* cids, const int32_t* Ts, const double* pose_mat,
                          const uint32_t* keep_mask, const double* next_pose, double* out) {
    OP_PROLOG(h);
    ARGCHK(h, V >= 1 && V <= PAM_MAX_VIEWS, "bad V");
    const int* c = S.in(cids, V); const int* t = S.in(Ts, V); const double* pm = S.in(pose_mat, (size_t)V * J3);
    const uint32_t* k = S.in(keep_mask, J); const double* np = S.in(next_pose, J3); double* o = S.out<double>(J3);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_dlt, dim3(1), dim3(64), 0, 0, camset(h), h->d_prm, V, c, t, pm, k, np, o);
    return S.finish(out, o, J3);
}

extern "C" int pam_op_dlt_paths(PamHandle* h, int V, const int32_t* cids, const int32_t* Ts, const double* pose_mat,
                                const uint32_t* keep_mask, const double* next_pose, int nsplit, int solver, double* out, int32_t* path) {
    OP_PROLOG(h);
    ARGCHK(h, V >= 1 && V <= PAM_MAX_VIEWS, "bad V");
    ARGCHK(h, (nsplit == 1 || nsplit == DLT_SPLIT) && (solver == 0 || solver == 1), "bad nsplit / solver");
    ARGCHK(h, cids && Ts && pose_mat && keep_mask && next_pose && out && path, "null argument");
    for (int v = 0; v < V; ++v) ARGCHK(h, cids[v] >= 0 && cids[v] < h->d.C, "camera id out of range");
    const int* c = S.in(cids, V); const int* t = S.in(Ts, V); const double* pm = S.in(pose_mat, (size_t)V * J3);
    const uint32_t* k = S.in(keep_mask, J); const double* np = S.in(next_pose, J3);
    double* part = S.out<double>((size_t)J * DLT_SPLIT * DLT_PACK); double* o = S.out<double>(J3); int* pp = S.out<int>(J);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_dlt_paths, dim3(1), dim3(64), 0, 0, camset(h), h->d_prm, V, c, t, pm, k, np, nsplit, solver, part, o, pp);
    return S.finish(out, o, J3, path, pp, J);
}

extern "C" int pam_op_smooth(PamHandle* h, int L, const double* hist, const double* raw, double* out) {
    if (!h) return PAM_E_ARG;
    OpStage S(h, __func__);
    ARGCHK(h, L >= 0 && L <= 4096, "bad L");
    const double* hs = S.in(hist, (size_t)(L > 0 ? L : 1) * J3); const double* r = S.in(raw, J3); double* o = S.out<double>(J3);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_smooth, dim3(1), dim3(64), 0, 0, h->d_prm, L, hs, r, o);
    return S.finish(out, o, J3);
}

extern "C" int pam_op_velocity(PamHandle* h, int L, const double* hist, float* vel) {
    if (!h) return PAM_E_ARG;
    OpStage S(h, __func__);
    ARGCHK(h, L >= 2 && L <= 4096, "bad L");
    const double* hs = S.in(hist, (size_t)L * J3); float* o = S.out<float>(J3);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_velocity, dim3(1), dim3(64), 0, 0, L, hs, o);
    return S.finish(vel, o, J3);
}

extern "C" int pam_op_hyp_cost(PamHandle* h, int n_members, const int32_t* cids, const double* poses, int o_cid,
                               const double* o_pose, double* cost, int32_t* veto) {
    OP_PROLOG(h);
    ARGCHK(h, n_members >= 1 && n_members <= PAM_MAX_VIEWS && o_cid >= 0 && o_cid < h->d.C, "bad members / camera");
    const int* c = S.in(cids, n_members); const double* ps = S.in(poses, (size_t)n_members * J3); const double* po = S.in(o_pose, J3);
    double* oc = S.out<double>(1); int* ov = S.out<int>(1);
    if (!S.staged()) return PAM_E_ARG;
    hipLaunchKernelGGL(k_op_hyp_cost, dim3(1), dim3(64), 0, 0, camset(h), h->d_prm, n_members, c, ps, o_cid, po, oc, ov);
    return S.finish(cost, oc, 1, veto, ov, 1);
}

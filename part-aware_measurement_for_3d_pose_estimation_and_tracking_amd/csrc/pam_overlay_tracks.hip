// libpam_hip.so, the overlay's primitive table built on the device from the tracker state (k_overlay_tracks) behind
// pam_overlay_tracks: every listed track's pose -- the One-Euro buffer's row or the newest of the history ring -- projected into every
// view of the call, a camera of the handle or an extra 3 x 4 matrix (the free-viewpoint 3D view), quantised to 1/8 pixel and written as
// the capsules pam_overlay_draw_counted paints (csrc/pam_overlay.hip).  The rules: include/pam.h; tests/overlay_tracks_ref.py restates
// them.  Reads the state only; one workgroup.  gfx950 only.
#include <string.h>
#include <math.h>
#include "pam_tracker.hpp"
#include "pam_lens.hpp"

#define OT_BLOCK 1024
#define OT_MAX_TRACKS 64              /* pam_create: at most 64 tracks */
#define OT_LIMBS 19
#define OT_ROWS (OT_LIMBS + J)        /* rows of one track in one view: the limbs, then the joints */
#define OT_COORD_MAX 262144.0         /* 2^18, in 1/8 pixel: what k_overlay takes */
static_assert(OT_ROWS == PAM_OVERLAY_TRACK_ROWS, "include/pam.h states the rows of a track");

// joints_dict()['coco']['skeleton'] of visualization.py, in its order
__device__ static const unsigned char OT_LIMB[OT_LIMBS][2] = {{15, 13}, {13, 11}, {16, 14}, {14, 12}, {11, 12}, {5, 11}, {6, 12},
                                                              {5, 6},   {5, 7},   {6, 8},   {7, 9},   {8, 10},  {1, 2},  {0, 1},
                                                              {0, 2},   {1, 3},   {2, 4},   {0, 5},   {0, 6}};

struct OtView { int32_t camera, extra, joint_hw, limb_hw; };
struct OtArgs {
    Dims d;
    const float* P;            // the handle's cameras, C x 12
    const char* state;
    const float* extra_P;      // n_extra x 12, or nullptr
    const double* pose;        // pam_one_euro's dev_pose of this scene (row i = list position i), or nullptr: the history ring's newest
    const double* lens;        // pam_set_lens: C rows of PAM_LENS_WORDS doubles, or nullptr
    OtView view[PAM_MAX_VIEWS];
    uint32_t palette[8 + J];
    int n_views, emitted_only, cap;
    PamOverlayPrim* prims;
    int32_t* count;
};
static_assert(sizeof(OtArgs) <= 4096, "descriptors travel in the kernel arguments");

// One joint in one view -> its coordinates in 1/8 pixel; false when it cannot be drawn (behind the camera, not finite, beyond 2^18).
__device__ __forceinline__ bool ot_joint(const float* __restrict__ P, const double* __restrict__ X, const double* __restrict__ lens,
                                         int camera, int& qx, int& qy) {
    const double h2 = (double)P[8] * X[0] + (double)P[9] * X[1] + (double)P[10] * X[2] + (double)P[11];
    if (!(h2 > 0.0)) return false;                                       // behind the camera, or NaN
    double u, w;
    project_point(P, X[0], X[1], X[2], u, w);
    if (lens) {                                                          // where the joint lies in the RAW image of this camera
        const Lens L = lens_row(lens, camera);
        if (!lens_is_pinhole(L)) {
            double x, y, xd, yd;
            lens_normalise(L, u, w, x, y);
            lens_forward(L, x, y, xd, yd);
            lens_pixels(L, xd, yd, u, w);
        }
    }
    const double fx = floor(8.0 * u + 0.5), fy = floor(8.0 * w + 0.5);   // NaN and infinities fail the comparisons below
    if (!(fabs(fx) <= OT_COORD_MAX) || !(fabs(fy) <= OT_COORD_MAX)) return false;
    qx = (int)fx; qy = (int)fy;
    return true;
}

__global__ __launch_bounds__(OT_BLOCK) void k_overlay_tracks(const OtArgs A) {
    __shared__ unsigned int s_joints[PAM_MAX_VIEWS * OT_MAX_TRACKS];          // drawable joints of (view, list position), one bit each
    __shared__ unsigned long long s_rows[PAM_MAX_VIEWS * OT_MAX_TRACKS];      // drawable rows: bits 0..18 the limbs, 19..35 the joints
    __shared__ int s_first[PAM_MAX_VIEWS * OT_MAX_TRACKS];                    // where the track's rows begin in its view's range
    __shared__ int s_total[PAM_MAX_VIEWS];
    __shared__ int s_slot[OT_MAX_TRACKS];                                     // list position -> slot, -1: not drawn
    __shared__ int s_newest[OT_MAX_TRACKS];
    const Dims d = A.d;
    const int HCAP = d.HCAP, tid = threadIdx.x, nV = A.n_views;
    SceneState st;
    carve_state(const_cast<char*>(A.state), d, st);
    const int nT = min(max(st.hdr[0], 0), min(d.MAXT, OT_MAX_TRACKS));
    for (int i = tid; i < nT; i += OT_BLOCK) {
        int s = st.order[i], newest = 0;
        if (s < 0 || s >= d.MAXT) s = -1;                                     // a state nobody should leave: nothing of it is indexed
        if (s >= 0 && A.emitted_only && !(st.tsu[s] == 0 && st.state[s] == CONFIRMED)) s = -1;
        if (s >= 0 && !A.pose) {
            newest = ring_newest(st, s, HCAP);
            if (st.h_len[s] < 1 || newest < 0 || newest >= HCAP) s = -1;
        }
        s_slot[i] = s; s_newest[i] = newest;
    }
    for (int it = tid; it < nV * nT; it += OT_BLOCK) s_joints[it] = 0u;
    __syncthreads();
    // 1: which joints can be drawn -- one lane per (view, track, joint)
    for (int it = tid; it < nV * nT * J; it += OT_BLOCK) {
        const int j = it % J, vi = it / J, i = vi % nT, v = vi / nT, s = s_slot[i];
        if (s < 0) continue;
        const OtView V = A.view[v];
        const float* P = V.camera >= 0 ? A.P + V.camera * 12 : A.extra_P + (size_t)V.extra * 12;
        const double* X = (A.pose ? A.pose + (size_t)i * J3 : st.hist + ((size_t)s * HCAP + s_newest[i]) * J3) + j * 3;
        int qx, qy;
        if (ot_joint(P, X, V.camera >= 0 ? A.lens : nullptr, V.camera, qx, qy)) atomicOr(&s_joints[vi], 1u << j);
    }
    __syncthreads();
    // 2: rows of every (view, track), then one lane per view walks the list: painter's order is list order
    for (int vi = tid; vi < nV * nT; vi += OT_BLOCK) {
        const unsigned int m = s_joints[vi];
        unsigned long long rows = (unsigned long long)m << OT_LIMBS;
        for (int l = 0; l < OT_LIMBS; ++l)
            if (((m >> OT_LIMB[l][0]) & 1u) && ((m >> OT_LIMB[l][1]) & 1u)) rows |= 1ull << l;
        s_rows[vi] = rows;
    }
    __syncthreads();
    for (int v = tid; v < nV; v += OT_BLOCK) {
        int run = 0;
        for (int i = 0; i < nT; ++i) { s_first[v * nT + i] = run; run += __popcll(s_rows[v * nT + i]); }
        s_total[v] = run;                                                     // <= 36 * nT <= cap
        A.count[v] = run;
    }
    __syncthreads();
    // 3: the rows -- one lane per (view, track, row); a limb projects its two joints again, a joint its one (the same expressions on
    //    the same inputs: the same bits as in step 1)
    for (int it = tid; it < nV * nT * OT_ROWS; it += OT_BLOCK) {
        const int r = it % OT_ROWS, vi = it / OT_ROWS, i = vi % nT, v = vi / nT;
        const unsigned long long rows = s_rows[vi];
        if (!((rows >> r) & 1ull)) continue;
        const int s = s_slot[i];
        const OtView V = A.view[v];
        const float* P = V.camera >= 0 ? A.P + V.camera * 12 : A.extra_P + (size_t)V.extra * 12;
        const double* lens = V.camera >= 0 ? A.lens : nullptr;
        const double* X = A.pose ? A.pose + (size_t)i * J3 : st.hist + ((size_t)s * HCAP + s_newest[i]) * J3;
        const bool limb = r < OT_LIMBS;
        const int ja = limb ? OT_LIMB[r][0] : r - OT_LIMBS, jb = limb ? OT_LIMB[r][1] : ja;
        int ax = 0, ay = 0, bx = 0, by = 0;
        ot_joint(P, X + ja * 3, lens, V.camera, ax, ay);
        if (limb) ot_joint(P, X + jb * 3, lens, V.camera, bx, by);
        else { bx = ax; by = ay; }
        const int id = st.track_id[s];
        const uint32_t bgr = limb ? A.palette[((id % 8) + 8) % 8] : A.palette[8 + ja];
        const int at = s_first[vi] + __popcll(rows & ((1ull << r) - 1ull));
        int4* o = reinterpret_cast<int4*>(A.prims + (size_t)v * A.cap + at);
        o[0] = make_int4(ax, ay, bx, by);
        o[1] = make_int4(limb ? V.limb_hw : V.joint_hw, (int)bgr, 0, 0);
    }
    // 4: every other row of every view's range is a null row
    for (int v = 0; v < nV; ++v) {
        for (int at = s_total[v] + tid; at < A.cap; at += OT_BLOCK) {
            int4* o = reinterpret_cast<int4*>(A.prims + (size_t)v * A.cap + at);
            o[0] = make_int4(0, 0, 0, 0);
            o[1] = make_int4(-1, 0, 0, 0);
        }
    }
}

// (joint radius, limb width) of a frame, visualization.overlay_style: rint rounds ties to even, as Python's round does
static void ot_style(int width, int height, int& radius, int& limb_width) {
    const int r = (int)rint((double)(width < height ? width : height) / 150.0);
    radius = r > 2 ? r : 2;
    limb_width = radius / 2 + 1;
}

// The primitive table of the tracks as the frame launches already on `stream` leave them (k_overlay_tracks).  Argument errors are
// answered before any device call.
extern "C" int pam_overlay_tracks(PamHandle* h, void* stream, int scene, int n_views, const PamOverlayTrackView* views,
                                  const float* dev_extra_P, int n_extra, const double* dev_pose, const uint32_t* palette, int emitted_only,
                                  int cap, PamOverlayPrim* dev_prims, int32_t* dev_count) {
    if (!h) return PAM_E_ARG;
    ARGCHK(h, views && palette && dev_prims && dev_count, "null buffer");
    ARGCHK(h, n_views >= 1 && n_views <= PAM_MAX_VIEWS, "n_views out of range");
    ARGCHK(h, n_extra >= 0 && (n_extra == 0 || dev_extra_P), "extra views without their matrices");
    ARGCHK(h, scene >= 0 && scene < h->d.S, "no such scene");
    ARGCHK(h, h->d.MAXT <= OT_MAX_TRACKS, "more track slots than the kernel holds");
    ARGCHK(h, cap >= PAM_OVERLAY_TRACK_ROWS * h->d.MAXT && cap <= (1 << 20), "cap below 36 rows per track slot (or above 2^20)");
    ARGCHK(h, ((uintptr_t)dev_prims & 15) == 0, "dev_prims is not 16-byte aligned");
    OtArgs A;
    memset(&A, 0, sizeof(A));
    for (int v = 0; v < n_views; ++v) {
        const PamOverlayTrackView& s = views[v];
        ARGCHK(h, s.camera >= -1 && s.camera < h->d.C, "no such camera");
        ARGCHK(h, s.camera >= 0 || (s.extra >= 0 && s.extra < n_extra), "no such extra view");
        ARGCHK(h, s.width >= 1 && s.width <= 65535 && s.height >= 1 && s.height <= 65535, "frame size out of range");
        int radius, limb_width;
        ot_style(s.width, s.height, radius, limb_width);
        A.view[v] = OtView{s.camera, s.camera >= 0 ? 0 : s.extra, 8 * radius, 4 * limb_width};
    }
    if (!h->cams_set) { h->err = "pam_set_cameras has not been called"; return PAM_E_STATE; }
    A.d = h->d; A.P = h->d_P; A.state = h->d_state + (size_t)scene * h->state_stride;
    A.extra_P = dev_extra_P; A.pose = dev_pose; A.lens = h->d_lens;
    for (int k = 0; k < 8 + J; ++k) A.palette[k] = palette[k];
    A.n_views = n_views; A.emitted_only = emitted_only ? 1 : 0; A.cap = cap;
    A.prims = dev_prims; A.count = dev_count;
    hipLaunchKernelGGL(k_overlay_tracks, dim3(1), dim3(OT_BLOCK), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return PAM_OK;
}

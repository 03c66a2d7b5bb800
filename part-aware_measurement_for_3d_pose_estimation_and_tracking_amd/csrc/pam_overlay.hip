// libpam_hip.so, the overlay of the tracked skeletons drawn into the frames on the device: limbs as capsules, joints as discs, in the
// integer arithmetic include/pam.h states (tests/overlay_ref.py restates it pixel for pixel).  One launch draws every view of a frame
// set; a workgroup owns a 64 x 16 pixel tile, culls its view's primitives against the tile into LDS, and leaves at once when none is
// left -- the usual case: a skeleton covers a few percent of a frame.  Painter's order: the last covering primitive of the table wins,
// so the culled list needs no order, a lane keeps the highest table index that covers its pixel.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/pam.h"

#define OV_BLOCK 256
#define OV_TILE_W 64                  /* a lane owns 4 consecutive pixels of a row: 12 consecutive bytes */
#define OV_TILE_H 16
#define OV_RUN 4
#define OV_LIST 512                   /* primitives of a view culled per pass; a longer table takes more passes */
#define OV_COORD_MAX (1 << 18)
#define OV_HW_MAX (1 << 12)

struct OvView {
    uint8_t* bgr;
    int32_t W, H, prim_first, prim_count;
    uint32_t wg_first, tiles_x;
};
struct OvArgs {
    OvView view[PAM_MAX_VIEWS];
    const PamOverlayPrim* prims;
    const int32_t* counts;            // pam_overlay_draw_counted: the views' primitive counts on the device, or nullptr
    int n_views;
};
static_assert(sizeof(OvArgs) <= 4096, "descriptors travel in the kernel arguments");

struct OvLds {
    int32_t ax, ay, bx, by, hw, index;
    uint32_t bgr;
};

__device__ __forceinline__ bool ov_inside(const OvLds& q, int64_t X, int64_t Y) {
    const int64_t dx = q.bx - q.ax, dy = q.by - q.ay, px = X - q.ax, py = Y - q.ay;
    const int64_t hw2 = (int64_t)q.hw * q.hw, dd = dx * dx + dy * dy, t = px * dx + py * dy;
    if (t <= 0) return px * px + py * py <= hw2;
    if (t >= dd) {
        const int64_t ex = X - q.bx, ey = Y - q.by;
        return ex * ex + ey * ey <= hw2;
    }
    const int64_t cr = px * dy - py * dx;
    if (cr <= -((int64_t)1 << 31) || cr >= ((int64_t)1 << 31)) return false;
    return cr * cr <= hw2 * dd;
}

__global__ __launch_bounds__(OV_BLOCK) void k_overlay(const OvArgs a) {
    __shared__ OvLds list[OV_LIST];
    __shared__ int n_list;
    int vi = 0;                                                           // workgroup-uniform: a workgroup never spans two views
    for (int k = 1; k < a.n_views; ++k)
        if (blockIdx.x >= a.view[k].wg_first) vi = k;
    const OvView& v = a.view[vi];
    const uint32_t tile = blockIdx.x - v.wg_first;
    const int ty = tile / v.tiles_x, tx = tile - ty * v.tiles_x;
    const int x_lo = tx * OV_TILE_W, y_lo = ty * OV_TILE_H;               // the tile in pixels, clipped to the frame
    const int x_hi = min(x_lo + OV_TILE_W, v.W) - 1, y_hi = min(y_lo + OV_TILE_H, v.H) - 1;
    const int y = y_lo + (int)(threadIdx.x >> 4), x0 = x_lo + (int)(threadIdx.x & 15) * OV_RUN;
    int best[OV_RUN];
    uint32_t colour[OV_RUN];
#pragma unroll
    for (int k = 0; k < OV_RUN; ++k) { best[k] = -1; colour[k] = 0; }
    // workgroup-uniform: a device count never reaches past the host's range of the table; a tile of a view that has 0 leaves at once
    const int prim_count = a.counts ? min(max(a.counts[vi], 0), v.prim_count) : v.prim_count;
    for (int base = 0; base < prim_count; base += OV_LIST) {
        if (threadIdx.x == 0) n_list = 0;
        __syncthreads();
        const int n = min(prim_count - base, OV_LIST);
        for (int i = threadIdx.x; i < n; i += OV_BLOCK) {
            const PamOverlayPrim p = a.prims[v.prim_first + base + i];
            if (abs(p.ax) > OV_COORD_MAX || abs(p.ay) > OV_COORD_MAX || abs(p.bx) > OV_COORD_MAX || abs(p.by) > OV_COORD_MAX || p.hw < 0 ||
                p.hw > OV_HW_MAX)
                continue;
            // the bounding box in 1/8 pixel against the tile's pixel centres: conservative, the exact test follows per pixel
            if (min(p.ax, p.bx) - p.hw > 8 * x_hi || max(p.ax, p.bx) + p.hw < 8 * x_lo || min(p.ay, p.by) - p.hw > 8 * y_hi ||
                max(p.ay, p.by) + p.hw < 8 * y_lo)
                continue;
            const int at = atomicAdd(&n_list, 1);
            list[at] = OvLds{p.ax, p.ay, p.bx, p.by, p.hw, base + i, p.bgr};
        }
        __syncthreads();
        const int m = n_list;
        if (y <= y_hi) {
            for (int j = 0; j < m; ++j) {
                const OvLds q = list[j];
#pragma unroll
                for (int k = 0; k < OV_RUN; ++k)
                    if (q.index > best[k] && ov_inside(q, 8 * (int64_t)(x0 + k), 8 * (int64_t)y)) { best[k] = q.index; colour[k] = q.bgr; }
            }
        }
        __syncthreads();                                                  // the list is rebuilt by the next pass
    }
    if (y > y_hi) return;
    uint8_t* const row = v.bgr + ((size_t)y * v.W + x0) * 3;
#pragma unroll
    for (int k = 0; k < OV_RUN; ++k)
        if (best[k] >= 0 && x0 + k <= x_hi) {
            row[3 * k] = (uint8_t)colour[k];
            row[3 * k + 1] = (uint8_t)(colour[k] >> 8);
            row[3 * k + 2] = (uint8_t)(colour[k] >> 16);
        }
}

static int ov_draw(void* stream, int n_views, const PamOverlayView* views, const PamOverlayPrim* dev_prims, int n_prims,
                   const int32_t* dev_count) {
    if (!views || n_views < 1 || n_views > PAM_MAX_VIEWS || n_prims < 0) return PAM_E_ARG;
    if (n_prims > 0 && (!dev_prims || ((uintptr_t)dev_prims & 15))) return PAM_E_ARG;
    OvArgs a;
    memset(&a, 0, sizeof(a));
    a.n_views = n_views;
    a.prims = dev_prims;
    a.counts = dev_count;
    uint64_t wg = 0;
    for (int i = 0; i < n_views; ++i) {
        const PamOverlayView& s = views[i];
        if (!s.dev_bgr || s.width < 1 || s.width > 65535 || s.height < 1 || s.height > 65535) return PAM_E_ARG;
        if (s.prim_first < 0 || s.prim_count < 0 || (int64_t)s.prim_first + s.prim_count > n_prims) return PAM_E_ARG;
        OvView& d = a.view[i];
        d.bgr = s.dev_bgr; d.W = s.width; d.H = s.height; d.prim_first = s.prim_first; d.prim_count = s.prim_count;
        d.tiles_x = (uint32_t)((s.width + OV_TILE_W - 1) / OV_TILE_W);
        d.wg_first = (uint32_t)wg;
        // a view without primitives gets no workgroup at all
        if (s.prim_count > 0) wg += (uint64_t)d.tiles_x * ((s.height + OV_TILE_H - 1) / OV_TILE_H);
    }
    if (wg == 0) return PAM_OK;
    hipLaunchKernelGGL(k_overlay, dim3((unsigned)wg), dim3(OV_BLOCK), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_overlay_draw(void* stream, int n_views, const PamOverlayView* views, const PamOverlayPrim* dev_prims, int n_prims) {
    return ov_draw(stream, n_views, views, dev_prims, n_prims, nullptr);
}

// the same launch with the views' counts read on the device (pam_overlay_tracks' dev_count)
extern "C" int pam_overlay_draw_counted(void* stream, int n_views, const PamOverlayView* views, const PamOverlayPrim* dev_prims, int n_prims,
                                        const int32_t* dev_count) {
    if (!dev_count) return PAM_E_ARG;
    return ov_draw(stream, n_views, views, dev_prims, n_prims, dev_count);
}

// The lens model of include/pam.h (Brown-Conrady, OpenCV / Panoptic order k1 k2 p1 p2 k3 on normalised coordinates; K upper-triangular
// with skew), float64, as device functions: shared by k_undistort_keypoints (pam_lens.hip) and k_track_boxes (pam_track_boxes.hip), so the
// boxes are drawn with the expressions the keypoints were undistorted with.  Built with -ffp-contract=off: every expression is
// evaluated as written.
#pragma once
#include <hip/hip_runtime.h>

#define PAM_LENS_WORDS 10     /* doubles of a camera's row: fx, fy, cx, cy, skew, k1, k2, p1, p2, k3 */
#define PAM_LENS_ITERS 8      /* Newton steps of the inverse: fixed, no data-dependent exit */
#define PAM_LENS_TOL 1e-9     /* largest residual of an inverted point, in normalised units */

namespace pam {

struct Lens { double fx, fy, cx, cy, skew, k1, k2, p1, p2, k3; };

__host__ __device__ __forceinline__ Lens lens_row(const double* __restrict__ table, long long g) {
    const double* r = table + g * PAM_LENS_WORDS;
    return Lens{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
}
// a camera whose five coefficients are all exactly zero is a pin-hole: its points are copied, never sent through K and back
__host__ __device__ __forceinline__ bool lens_is_pinhole(const Lens& L) {
    return L.k1 == 0.0 && L.k2 == 0.0 && L.p1 == 0.0 && L.p2 == 0.0 && L.k3 == 0.0;
}
// pixels (u = column, w = row) <-> normalised coordinates
__host__ __device__ __forceinline__ void lens_normalise(const Lens& L, double u, double w, double& x, double& y) {
    y = (w - L.cy) / L.fy;
    x = (u - L.cx - L.skew * y) / L.fx;
}
__host__ __device__ __forceinline__ void lens_pixels(const Lens& L, double x, double y, double& u, double& w) {
    u = L.fx * x + L.skew * y + L.cx;
    w = L.fy * y + L.cy;
}
// forward model, closed form: ideal (x, y) -> distorted (xd, yd)
__host__ __device__ __forceinline__ void lens_forward(const Lens& L, double x, double y, double& xd, double& yd) {
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3));
    xd = x * rad + 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * x * x);
    yd = y * rad + L.p1 * (r2 + 2.0 * y * y) + 2.0 * L.p2 * x * y;
}
// inverse: Newton on the 2 x 2 system with the analytic Jacobian, from the distorted point, PAM_LENS_ITERS steps.  -> false when an
// iterate's Jacobian determinant is <= 0 (or NaN) or the final residual exceeds PAM_LENS_TOL in either coordinate (x, y are then not to
// be used).  A failed iterate does not end the loop: every lane runs the same PAM_LENS_ITERS steps.
__host__ __device__ __forceinline__ bool lens_inverse(const Lens& L, double dx, double dy, double& x, double& y) {
    bool ok = true;
    x = dx; y = dy;
    for (int it = 0; it < PAM_LENS_ITERS; ++it) {
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3));
        const double drad = L.k1 + r2 * (2.0 * L.k2 + 3.0 * r2 * L.k3);            // d rad / d r2
        const double ex = x * rad + 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * x * x) - dx;
        const double ey = y * rad + L.p1 * (r2 + 2.0 * y * y) + 2.0 * L.p2 * x * y - dy;
        const double a = rad + 2.0 * x * x * drad + 2.0 * L.p1 * y + 6.0 * L.p2 * x;     // d xd / d x
        const double b = 2.0 * x * y * drad + 2.0 * L.p1 * x + 2.0 * L.p2 * y;            // d xd / d y = d yd / d x
        const double d = rad + 2.0 * y * y * drad + 6.0 * L.p1 * y + 2.0 * L.p2 * x;     // d yd / d y
        const double det = a * d - b * b;
        if (!(det > 0.0)) ok = false;
        x = x - (d * ex - b * ey) / det;
        y = y - (a * ey - b * ex) / det;
    }
    double fx, fy;
    lens_forward(L, x, y, fx, fy);
    if (!(fabs(fx - dx) <= PAM_LENS_TOL) || !(fabs(fy - dy) <= PAM_LENS_TOL)) ok = false;
    return ok;
}

}  // namespace pam

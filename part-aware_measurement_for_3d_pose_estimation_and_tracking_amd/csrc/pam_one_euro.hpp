// The One-Euro filter's step on one scalar channel (include/pam.h, pam_one_euro; OneEuroFilter.__call__ of the reference, float64
// throughout): shared by k_one_euro and the parity kernel behind pam_op_one_euro.  The library is built with -ffp-contract=off, so every
// line below is computed as written.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/pam.h"

namespace pam {

#define PAM_OE_PI 3.141592653589793

// the sampling frequency a filter with n samples behind it takes for a sample at time t (the class's truthiness test: a time stamp of
// 0.0 counts as "none")
__device__ __forceinline__ double one_euro_freq(int n, double freq, double t_last, double t) {
    return (n > 0 && t_last != 0.0 && t != 0.0) ? 1.0 / (t - t_last) : freq;
}

__device__ __forceinline__ double one_euro_alpha(double freq, double cutoff) {
    const double te = 1.0 / freq;
    const double tau = 1.0 / (2 * PAM_OE_PI * cutoff);
    return 1.0 / (1.0 + tau / te);
}

// One step of one channel.  n, freq, t_last: the filter's header BEFORE this sample (the caller stores n + 1, one_euro_freq(...) and t
// afterwards; the 51 channels of a track share them).  x_prev, x_hat, dx_hat: the channel's own state, updated.  -> x_hat.
__device__ __forceinline__ double one_euro_step(const PamOneEuro& c, int n, double freq, double t_last, double t, double x,
                                                double& x_prev, double& x_hat, double& dx_hat) {
    const double f = one_euro_freq(n, freq, t_last, t);
    double edx = 0.0, out = x;                                           // the first sample: no derivative, the output is the input's bits
    if (n != 0) {
        const double dx = (x - x_prev) * f;
        const double ad = one_euro_alpha(f, c.dcutoff);
        edx = ad * dx + (1.0 - ad) * dx_hat;
    }
    const double cut = c.mincutoff + c.beta * fabs(edx);
    if (n != 0) {
        const double ax = one_euro_alpha(f, cut);
        out = ax * x + (1.0 - ax) * x_hat;
    }
    dx_hat = edx; x_prev = x; x_hat = out;
    return out;
}

}  // namespace pam

// rope_solve.h — what the two native polish files (rope_polish.hip, rope_bundle_polish.hip) have in common, once: THE ELIMINATION
// of include/rope_s3d.h on systems that lie in LDS element-major, the clip to the joint limits, the mean truncated cost of a
// system's words, and the host checks of masks, limits and pointers.  Everything is float64 with one IEEE operation per written
// operation (-ffp-contract=off, no fma); tests/polish_ref.py and tests/bundle_polish_ref.py hold the callers to it bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

namespace {

#define EL(r, c) s_m[(r) * RW + (c)][t]

// Gaussian elimination with partial pivoting and back substitution of a p x p system with nr right-hand sides: element (r, c) of M
// at s_m[r RW + c][t], right-hand side m at column MW + m; t is the thread's column of s_m (TS threads a workgroup share it, lane t
// reads word t of a row of consecutive words whatever element its own control flow has reached).  The pivot search indexes rows at
// run time, which is why the systems lie in LDS: a per-thread array indexed that way would live in scratch.  Every row operation
// goes over all right-hand sides; x replaces them.  false: SINGULAR, a pivot that is 0 or not finite.
template <int MW, int RW, int TS>
__device__ __forceinline__ bool eliminate(double (*s_m)[TS], int t, int p, int nr)
{
    for (int k = 0; k < p; k++) {
        int piv = k;
        double best = fabs(EL(k, k));
        for (int r = k + 1; r < p; r++) {                       // the FIRST row with the largest magnitude
            const double a = fabs(EL(r, k));
            if (a > best) { best = a; piv = r; }
        }
        const double pv = EL(piv, k);
        if (pv == 0.0 || !isfinite(pv)) return false;
        if (piv != k) {
            for (int c = k; c < p; c++) { const double u = EL(k, c); EL(k, c) = EL(piv, c); EL(piv, c) = u; }
            for (int m = 0; m < nr; m++) { const double u = EL(k, MW + m); EL(k, MW + m) = EL(piv, MW + m); EL(piv, MW + m) = u; }
        }
        for (int i = k + 1; i < p; i++) {
            const double f = EL(i, k) / pv;
            for (int c = k + 1; c < p; c++) EL(i, c) = EL(i, c) - f * EL(k, c);
            for (int m = 0; m < nr; m++) EL(i, MW + m) = EL(i, MW + m) - f * EL(k, MW + m);
        }
    }
    for (int m = 0; m < nr; m++)
        for (int i = p - 1; i >= 0; i--) {
            double s = EL(i, MW + m);
            for (int c = i + 1; c < p; c++) s = s - EL(i, c) * EL(c, MW + m);
            EL(i, MW + m) = s / EL(i, i);
        }
    return true;
}

// whether all of x is finite
template <int MW, int RW, int TS>
__device__ __forceinline__ bool all_finite(double (*s_m)[TS], int t, int p, int nr)
{
    bool ok = true;
    for (int r = 0; r < p; r++)
        for (int m = 0; m < nr; m++) ok = ok && isfinite(EL(r, MW + m));
    return ok;
}

#undef EL

__device__ __forceinline__ double clip_to(double v, double lo, double hi)
{
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// the mean truncated cost of a system's words, a frame's or the pool's: [1] / [0], inf without a pixel to compare
__device__ __forceinline__ double mean_cost(const double *w) { return w[0] > 0.0 ? w[1] / w[0] : (double)INFINITY; }

// The six joints' limits as a kernel argument, from the ABI's (lo, hi) pairs; bad_limits says whether those may be taken
struct JointLimits {
    double lo[6], hi[6];
    explicit JointLimits(const double *limits)
    {
        for (int j = 0; j < 6; j++) { lo[j] = limits[2 * j]; hi[j] = limits[2 * j + 1]; }
    }
};

inline bool bad_limits(const double *limits)
{
    if (!limits) return true;
    for (int j = 0; j < 6; j++)
        if (!std::isfinite(limits[2 * j]) || !std::isfinite(limits[2 * j + 1]) || limits[2 * j] > limits[2 * j + 1]) return true;
    return false;
}
inline bool bad_mask6(int mask) { return mask < 0 || mask > 63; }              // a bit a joint, or a camera parameter
inline bool misaligned8(const void *p) { return ((uintptr_t)p & 7) != 0; }

}  // namespace

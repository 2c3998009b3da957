// rope_fk.h — the forward-kinematics chain of the device, shared by every kernel that needs a link's transform: the deterministic
// float64 sine / cosine, the 3x4 affine product and a joint's matrix.  rope_kernels.hip (fk_mvp_kernel and the kernels that do their
// own forward kinematics) and rope_polish.hip (joint_axes_kernel) include this one text, so their chains agree bit for bit;
// oracle/ mirrors it on the CPU (oracle.sincos, Oracle.fk).  One IEEE operation per written operation (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

namespace rope {

// ------------------------------------------------------------------ sincos -----
// Cody-Waite reduction by pi/2 + msun kernel polynomials, <= 1 ulp of libm.
__device__ static inline double k_sin(double x, double y)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    double z = x * x, w = z * z;
    double r = (S2 + z * (S3 + z * S4)) + (z * w) * (S5 + z * S6);
    double v = z * x;
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

__device__ static inline double k_cos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double z = x * x, w = z * z;
    double r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
    double hz = 0.5 * z;
    double ww = 1.0 - hz;
    return ww + (((1.0 - ww) - hz) + (z * r - x * y));
}

__device__ static inline void det_sincos(double x, double &s, double &c)
{
    const double PIO2_1 = 1.57079632673412561417e+00, PIO2_1T = 6.07710050650619224932e-11;
    const double INV_PIO2 = 6.36619772367581382433e-01;
    double fn = rint(x * INV_PIO2);
    double r = x - fn * PIO2_1;
    double w = fn * PIO2_1T;
    double y0 = r - w;
    double y1 = (r - y0) - w;
    int n = (int)((long long)fn & 3);
    double sn = k_sin(y0, y1), cs = k_cos(y0, y1);
    s = (n == 0) ? sn : (n == 1) ? cs : (n == 2) ? -sn : -cs;
    c = (n == 0) ? cs : (n == 1) ? -sn : (n == 2) ? -cs : sn;
}

// ------------------------------------------------------------------- FK --------
__device__ static inline void aff_mul(const double *A, const double *B, double *O)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            O[4 * r + c] = (A[4 * r + 0] * B[0 + c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
        O[4 * r + 3] = ((A[4 * r + 0] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
    }
}

// A_j = F_j · Rot(axis_j, q_j): parent-link frame -> link j+1 frame (12 doubles, 3x4 row-major)
__device__ static inline void joint_matrix(double q, int j, const double *__restrict__ joint_fixed, const double *__restrict__ joint_axes,
                                           double *A)
{
    double s, co;
    det_sincos(q, s, co);
    const double t = 1.0 - co, ax = joint_axes[3 * j], ay = joint_axes[3 * j + 1], az = joint_axes[3 * j + 2];
    double R[12], F[12];
    R[0] = (t * ax) * ax + co;      R[1] = (t * ax) * ay - s * az;  R[2] = (t * ax) * az + s * ay;  R[3] = 0.0;
    R[4] = (t * ax) * ay + s * az;  R[5] = (t * ay) * ay + co;      R[6] = (t * ay) * az - s * ax;  R[7] = 0.0;
    R[8] = (t * ax) * az - s * ay;  R[9] = (t * ay) * az + s * ax;  R[10] = (t * az) * az + co;     R[11] = 0.0;
#pragma unroll
    for (int k = 0; k < 12; k++) F[k] = joint_fixed[12 * j + k];
    aff_mul(F, R, A);
}

}  // namespace rope

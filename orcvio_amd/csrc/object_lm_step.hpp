// object_lm_step.hpp -- what the two object optimisers have in common as code: k_object_lm (object_lm.hpp: one workgroup per
// object, thread 0 solves the 9 x 9 head out of LDS) and k_object_lm_lite (object_lite.hpp: one wavefront per object, every lane solves
// the 9 x 9 system in its own registers).  Shared here: the accumulator count, the status codes, the index of the packed upper
// triangle and the SE(3) exponential.  NOT shared -- written out in both kernels, in the same expression order, and to be changed in
// both: the evaluation arguments, the 55-accumulator update, the damped 9 x 9 Cholesky with its solves, the predicted decrease, the
// 4 x 4 retraction, the rho / lambda rule and the skip-word output.  Each was tried behind an inlined helper and taken out again: the
// retraction changed which multiply-adds the compiler fuses in both kernels; the Cholesky and the predicted decrease left
// k_object_lm_lite computing other bits (11 of 106 result digests); the rest kept k_object_lm_lite's code but moved k_object_lm's
// scalar registers and addressing, and a kernel whose code differs from what was measured and profiled has to earn that.
// tests/test_gpu_object_lite.py and test_gpu_object_init.py pin the two kernels' agreement with their one-call forms bit for bit.
#pragma once
#include "object_rows.hpp"

namespace orcvio_amd {

#define OBJ_LM_ACC 55           // per-lane accumulators: 45 products of nine columns (upper triangle by rows), 9 gradient entries, the cost

// the per-object status of an optimiser (include/orcvio_msckf.h); 0 is the skip word's: not optimised
#define OBJ_LM_ST_CONVERGED 1
#define OBJ_LM_ST_STALLED 2
#define OBJ_LM_ST_ITER_CAP 3
#define OBJ_LM_ST_NONFINITE 4

__device__ __forceinline__ int obj_lm_sym(int i, int j) { return i * 9 - i * (i - 1) / 2 + (j - i); }   // i <= j, upper triangle by rows

// Sophus SE3d::exp, tangent (upsilon, omega): R = exp(omega), t = V upsilon (the thresholds of oracle/mirror_objects.se3_exp)
__device__ inline void obj_lm_se3_exp(const double* xi, double* T) {
    const double* u = xi;
    const double* w = xi + 3;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double W2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
    double a, b, ra, rb;
    if (th < 1e-10) { ra = 1.0; rb = 0.5; a = 0.5; b = 1.0 / 6.0; }
    else {
        const double s = sin(th), c = cos(th);
        ra = s / th; rb = (1.0 - c) / th2; a = rb; b = (th - s) / (th2 * th);
    }
    for (int i = 0; i < 3; ++i) {
        double V[3];
        for (int j = 0; j < 3; ++j) {
            const double e = (i == j) ? 1.0 : 0.0;
            T[4 * i + j] = e + ra * W[3 * i + j] + rb * W2[3 * i + j];
            V[j] = e + a * W[3 * i + j] + b * W2[3 * i + j];
        }
        T[4 * i + 3] = V[0] * u[0] + V[1] * u[1] + V[2] * u[2];
    }
    T[12] = T[13] = T[14] = 0.0; T[15] = 1.0;
}

}  // namespace orcvio_amd

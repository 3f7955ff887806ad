// object_init.hpp -- the start of an object track on the device: linear triangulation of every keypoint over the track's frames,
// Kabsch alignment of the mean keypoints onto the triangulated ones, the pose in one of three rigid forms.
// Reference: ObjectFeatureInitializer::single_object_initialization (src/obj/ObjectFeatureInitializer.cpp:33-198) over
// single_triangulation_common (src/feat/FeatureInitializer.cpp:6-111), findTransform (:265-344) and poseSE32SE2
// (include/orcvio/utils/se3_ops.hpp:272-300).
//
// One workgroup per object, as k_object_lm; it reads the optimiser's staged block (object_mapper_pack.hpp) and writes the start -- its
// pose, the mean shape, the mean keypoints -- into the block's first 19 + 3K doubles, so k_object_lm can follow on the same stream.
// Triangulation: wavefront w takes keypoints w, w + 4, ..; lane <-> frame, a second pass for frames 64..127.  Each row pair
//   Bperp_i = [-b2 0 b0; 0 b2 -b1],  b = R_AtoCi^T (u, v, 1) / |.|
// adds to A^T A = [s22 0 -s02; 0 s22 -s12; -s02 -s12 s00 + s11] and A^T (Bperp_i p_CiinA): seven wave sums (tri_wave_sum), a 3 x 3
// Cholesky, and cond(A) = sqrt of the ratio of the extreme eigenvalues of A^T A (one-sided Jacobi on the symmetric matrix).
// Alignment: one lane, K <= 16 points from LDS; the 3 x 3 SVD is a one-sided Jacobi with a fixed number of sweeps.
// No workgroup waits for another; every loop is bounded by K, by the two frame passes or by OBJ_INIT_SWEEPS.
#pragma once
#include "object_mapper_pack.hpp"   // the layout of the staged blocks
#include "triangulate.hpp"        // tri_wave_sum

namespace orcvio_amd {

#define OBJ_INIT_NT 256           // threads per workgroup (four wavefronts)
#define OBJ_INIT_SWEEPS 12        // one-sided Jacobi on 3 x 3: quadratic convergence, five or six sweeps reach rounding

struct ObjInitArgs {
    ObjLmTrack* tracks;           // pad <- 1 where the optimiser must skip the object (status other than 1)
    double* in;                   // the staged input block; the start of every track is written
    double* out;                  // [n_tracks][OBJ_INIT_OUT]
    int pose_form, min_obs, min_kps;
};

// A (row-major) = U diag(s) V^T with s descending: one-sided Jacobi (Hestenes) on the columns, a fixed number of sweeps.  U's third
// column is u0 x u1 (det U = +1): a column of a rank-2 matrix has no direction of its own, and R = V diag(1, 1, d) U^T does not
// depend on its sign.
__device__ __forceinline__ void obj_init_svd3(const double* A, double* U, double* s, double* V) {
    double g0[3], g1[3], g2[3], v0[3] = {1, 0, 0}, v1[3] = {0, 1, 0}, v2[3] = {0, 0, 1};
#pragma unroll
    for (int i = 0; i < 3; ++i) { g0[i] = A[3 * i]; g1[i] = A[3 * i + 1]; g2[i] = A[3 * i + 2]; }
    auto rotate = [](double* gp, double* gq, double* vp, double* vq) {
        const double alpha = gp[0] * gp[0] + gp[1] * gp[1] + gp[2] * gp[2];
        const double beta = gq[0] * gq[0] + gq[1] * gq[1] + gq[2] * gq[2];
        const double gamma = gp[0] * gq[0] + gp[1] * gq[1] + gp[2] * gq[2];
        if (gamma != 0.0) {
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double a = gp[i], b = gq[i];
                gp[i] = c * a - sn * b; gq[i] = sn * a + c * b;
                const double va = vp[i], vb = vq[i];
                vp[i] = c * va - sn * vb; vq[i] = sn * va + c * vb;
            }
        }
    };
    for (int sweep = 0; sweep < OBJ_INIT_SWEEPS; ++sweep) {
        rotate(g0, g1, v0, v1);
        rotate(g0, g2, v0, v2);
        rotate(g1, g2, v1, v2);
    }
    double n0 = g0[0] * g0[0] + g0[1] * g0[1] + g0[2] * g0[2];
    double n1 = g1[0] * g1[0] + g1[1] * g1[1] + g1[2] * g1[2];
    double n2 = g2[0] * g2[0] + g2[1] * g2[1] + g2[2] * g2[2];
    auto order = [](double& na, double& nb, double* ga, double* gb, double* va, double* vb) {
        if (na < nb) {
            double x = na; na = nb; nb = x;
#pragma unroll
            for (int i = 0; i < 3; ++i) { x = ga[i]; ga[i] = gb[i]; gb[i] = x; x = va[i]; va[i] = vb[i]; vb[i] = x; }
        }
    };
    order(n0, n1, g0, g1, v0, v1);
    order(n1, n2, g1, g2, v1, v2);
    order(n0, n1, g0, g1, v0, v1);
    s[0] = sqrt(n0); s[1] = sqrt(n1); s[2] = sqrt(n2);
    const double i0 = 1.0 / s[0], i1 = 1.0 / s[1];
    double u0[3], u1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { u0[i] = g0[i] * i0; u1[i] = g1[i] * i1; }
    const double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        U[3 * i] = u0[i]; U[3 * i + 1] = u1[i]; U[3 * i + 2] = u2[i];
        V[3 * i] = v0[i]; V[3 * i + 1] = v1[i]; V[3 * i + 2] = v2[i];
    }
}

__global__ __launch_bounds__(OBJ_INIT_NT) void k_object_init(ObjInitArgs a) {
    __shared__ double sP[OBJ_LM_MAXK][3];   // the triangulated keypoints (world)
    __shared__ int sUsed[OBJ_LM_MAXK];
    __shared__ int sStatus;

    const int o = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ObjLmTrack tr = a.tracks[o];
    const int K = tr.K, F = tr.F;
    double* blk = a.in + tr.off;
    const double* mean_kps = blk + 22 + 3 * K;
    const double* wTc = blk + 22 + 6 * K;
    const double* zs = wTc + (size_t)16 * F;
    double* out = a.out + (size_t)o * OBJ_INIT_OUT;
    const int npass = (F + 63) >> 6;        // one pass, or two for frames 64..127
    const double qnan = __builtin_nan("");

    for (int k = wave; k < OBJ_LM_MAXK; k += OBJ_INIT_NT / 64) {   // (wave-uniform: every lane reaches the ballots and the wave sums)
        int cnt = 0, anchor = 0;
        double u[2], v[2];
        bool det[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int f = 64 * p + lane;
            det[p] = false; u[p] = 0.0; v[p] = 0.0;
            if (p < npass && k < K) {
                if (f < F) {
                    u[p] = zs[((size_t)f * K + k) * 2]; v[p] = zs[((size_t)f * K + k) * 2 + 1];
                    det[p] = isfinite(u[p]) && isfinite(v[p]);
                }
                const unsigned long long m = __ballot(det[p]);
                cnt += __popcll(m);
                if (m != 0ull) anchor = 64 * p + 63 - __clzll((long long)m);   // the LAST frame with a detection
            }
        }
        const bool used = k < K && cnt > a.min_obs && cnt > 0;
        double P[3] = {qnan, qnan, qnan}, cond = qnan;
        if (used) {
            const double* Ta = wTc + (size_t)16 * anchor;   // camera -> world of the anchor: R_GtoA = Ra^T, p_AinG = ta
            const double Ra[9] = {Ta[0], Ta[1], Ta[2], Ta[4], Ta[5], Ta[6], Ta[8], Ta[9], Ta[10]};
            const double ta[3] = {Ta[3], Ta[7], Ta[11]};
            double acc[7] = {0, 0, 0, 0, 0, 0, 0};   // s22, s02, s12, s00 + s11, A^T b
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (det[p]) {
                    const double* Ti = wTc + (size_t)16 * (64 * p + lane);
                    // b = R_AtoCi^T (u, v, 1) = Ra^T (Ri (u, v, 1)), normalised; p_CiinA = Ra^T (ti - ta)
                    double w[3], d[3], b[3], pc[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) { w[i] = Ti[4 * i] * u[p] + Ti[4 * i + 1] * v[p] + Ti[4 * i + 2]; d[i] = Ti[4 * i + 3] - ta[i]; }
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        b[i] = Ra[i] * w[0] + Ra[3 + i] * w[1] + Ra[6 + i] * w[2];
                        pc[i] = Ra[i] * d[0] + Ra[3 + i] * d[1] + Ra[6 + i] * d[2];
                    }
                    const double inv = 1.0 / sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
                    b[0] *= inv; b[1] *= inv; b[2] *= inv;
                    const double c1 = b[0] * pc[2] - b[2] * pc[0], c2 = b[2] * pc[1] - b[1] * pc[2];   // Bperp p_CiinA
                    acc[0] += b[2] * b[2]; acc[1] += b[0] * b[2]; acc[2] += b[1] * b[2]; acc[3] += b[0] * b[0] + b[1] * b[1];
                    acc[4] += -b[2] * c1; acc[5] += b[2] * c2; acc[6] += b[0] * c1 - b[1] * c2;
                }
            }
#pragma unroll
            for (int i = 0; i < 7; ++i) acc[i] = tri_wave_sum(acc[i]);
            // (A^T A) x = A^T b by Cholesky: [s22 0 -s02; 0 s22 -s12; -s02 -s12 s00 + s11]
            const double l00 = sqrt(acc[0]), i00 = 1.0 / l00;
            const double l20 = -acc[1] * i00, l21 = -acc[2] * i00;
            const double l22 = sqrt(acc[3] - l20 * l20 - l21 * l21), i22 = 1.0 / l22;
            const double y0 = acc[4] * i00, y1 = acc[5] * i00, y2 = (acc[6] - l20 * y0 - l21 * y1) * i22;
            const double x2 = y2 * i22, x0 = (y0 - l20 * x2) * i00, x1 = (y1 - l21 * x2) * i00;
#pragma unroll
            for (int i = 0; i < 3; ++i) P[i] = Ra[3 * i] * x0 + Ra[3 * i + 1] * x1 + Ra[3 * i + 2] * x2 + ta[i];   // R_GtoA^T p_FinA + p_AinG
            const double M[9] = {acc[0], 0.0, -acc[1], 0.0, acc[0], -acc[2], -acc[1], -acc[2], acc[3]};
            double Um[9], sm[3], Vm[9];
            obj_init_svd3(M, Um, sm, Vm);
            cond = sqrt(sm[0] / sm[2]);
        }
        if (lane == 0) {
            sUsed[k] = used ? 1 : 0;
            sP[k][0] = P[0]; sP[k][1] = P[1]; sP[k][2] = P[2];
            out[OBJ_INIT_O_KPS + 3 * k] = P[0]; out[OBJ_INIT_O_KPS + 3 * k + 1] = P[1]; out[OBJ_INIT_O_KPS + 3 * k + 2] = P[2];
            out[OBJ_INIT_O_USED + k] = used ? 1.0 : 0.0;
            out[OBJ_INIT_O_OBS + k] = (double)cnt;
            out[OBJ_INIT_O_COND + k] = cond;
        }
    }
    __syncthreads();

    if (tid == 0) {
        double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        double R[9] = {qnan, qnan, qnan, qnan, qnan, qnan, qnan, qnan, qnan}, t[3] = {qnan, qnan, qnan}, sg[3] = {qnan, qnan, qnan};
        double scale = qnan;
        int n = 0, status = 2;
        for (int k = 0; k < K; ++k) n += sUsed[k];
        if (n > a.min_kps && n > 0) {
            // the scale: summed chords between consecutive used keypoints; the centroids (out already divided by the scale)
            double din = 0.0, dout = 0.0, ci[3] = {0, 0, 0}, co[3] = {0, 0, 0}, pi[3] = {0, 0, 0}, po[3] = {0, 0, 0};
            bool first = true;
            for (int k = 0; k < K; ++k) {
                if (!sUsed[k]) continue;
                const double xi[3] = {mean_kps[3 * k], mean_kps[3 * k + 1], mean_kps[3 * k + 2]};
                const double xo[3] = {sP[k][0], sP[k][1], sP[k][2]};
                if (!first) {
                    din += sqrt((xi[0] - pi[0]) * (xi[0] - pi[0]) + (xi[1] - pi[1]) * (xi[1] - pi[1]) + (xi[2] - pi[2]) * (xi[2] - pi[2]));
                    dout += sqrt((xo[0] - po[0]) * (xo[0] - po[0]) + (xo[1] - po[1]) * (xo[1] - po[1]) + (xo[2] - po[2]) * (xo[2] - po[2]));
                }
                first = false;
#pragma unroll
                for (int i = 0; i < 3; ++i) { pi[i] = xi[i]; po[i] = xo[i]; ci[i] += xi[i]; co[i] += xo[i]; }
            }
            scale = dout / din;
            double cs[3];           // centroid of out / scale
            {
                double acc3[3] = {0, 0, 0};
                for (int k = 0; k < K; ++k) {
                    if (!sUsed[k]) continue;
#pragma unroll
                    for (int i = 0; i < 3; ++i) acc3[i] += sP[k][i] / scale;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) { cs[i] = acc3[i] / (double)n; ci[i] /= (double)n; co[i] /= (double)n; }
            }
            double Cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < K; ++k) {
                if (!sUsed[k]) continue;
                double xi[3], xo[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) { xi[i] = mean_kps[3 * k + i] - ci[i]; xo[i] = sP[k][i] / scale - cs[i]; }
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) Cov[3 * i + j] += xi[i] * xo[j];
            }
            double U[9], V[9];
            obj_init_svd3(Cov, U, sg, V);
            // d = sign det(V U^T) = sign det V (det U = +1);  R = V diag(1, 1, d) U^T
            const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
            const double dd = detV > 0.0 ? 1.0 : -1.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) R[3 * i + j] = V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1] + dd * V[3 * i + 2] * U[3 * j + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = scale * (cs[i] - (R[3 * i] * ci[0] + R[3 * i + 1] * ci[1] + R[3 * i + 2] * ci[2]));
            bool finite = isfinite(scale);
#pragma unroll
            for (int i = 0; i < 9; ++i) finite = finite && isfinite(R[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) finite = finite && isfinite(t[i]) && isfinite(sg[i]);
            status = finite ? 1 : 4;
            if (finite) {
                if (a.pose_form == 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2];
                        T[4 * i + 3] = co[i] - (R[3 * i] * ci[0] + R[3 * i + 1] * ci[1] + R[3 * i + 2] * ci[2]);
                    }
                } else {
                    const double at = atan2(scale * R[3], scale * R[0]);
                    double yaw = a.pose_form == 1 ? M_PI / at : at;
                    if (!isfinite(yaw)) yaw = 0.0;
                    const double c = cos(yaw), sn = sin(yaw);
                    T[0] = c; T[1] = -sn; T[3] = t[0];
                    T[4] = sn; T[5] = c; T[7] = t[1];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) { out[i] = T[i]; blk[i] = T[i]; }
#pragma unroll
        for (int i = 0; i < 9; ++i) out[OBJ_INIT_O_R + i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { out[OBJ_INIT_O_T + i] = t[i]; out[OBJ_INIT_O_SIGMA + i] = sg[i]; }
        out[OBJ_INIT_O_SCALE] = scale;
        out[OBJ_INIT_O_NUSED] = (double)n;
        out[OBJ_INIT_O_STATUS] = (double)status;
        a.tracks[o].pad = status == 1 ? 0 : 1;
    }
    // the rest of the optimiser's start: the mean shape and the mean keypoints (the reference's LMObjectState)
    for (int i = tid; i < 3 + 3 * K; i += OBJ_INIT_NT) blk[16 + i] = blk[19 + 3 * K + i];
}

}  // namespace orcvio_amd

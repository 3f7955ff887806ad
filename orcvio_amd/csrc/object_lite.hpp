// object_lite.hpp -- the lite (bbox-only) object mapper on the device: the start of a track from its first bounding box and the
// batched Levenberg-Marquardt over the state x = (wTo in SE(3), shape v), 9 degrees of freedom [pose 6 | shape 3].
// Reference: ObjectFeatureInitializer::single_object_initialization_lite (src/obj/ObjectFeatureInitializer.cpp:495-584) and
// single_levenberg_marquardt_lite (:442-493) over the ObjectLMLite functor (src/obj/ObjectLMLite.cpp:389-415): w0 x the four bbox
// rows of every frame, w1 x (v - mean_shape) repeated F - 1 times (include/orcvio/obj/ObjectLMLite.h:288-297), Huber off.  The
// iteration is the one documented in include/orcvio_msckf.h for orcvio_msckf_object_lm.
//
// k_object_lm_lite: one WAVEFRONT per object, four objects per workgroup.  A lane owns one (frame, line) pair, 16 frames per pass
// (object_rows_lane_at with four lanes per frame: the body k_object_rows, k_obj_fused and k_object_lm evaluate), and keeps the 45
// products, the 9 gradient entries and the cost of its rows in registers.  A butterfly over the 64 lanes (xor 1, 2, .. 32: a fixed
// order) leaves EVERY lane with the same sums, bit for bit; from there every lane carries the whole iteration redundantly in its own
// registers -- the regulariser (w1^2 x repeats on the diagonal and the gradient: no rows), the 9 x 9 Cholesky of the damped system,
// the retraction, the rho rule -- so the lanes of a wavefront agree on every branch without exchanging a word.
// The wavefronts of a workgroup run different objects with different iteration counts: the kernel contains NO __syncthreads() and NO
// LDS at all; nothing a wavefront needs comes from another.  Every loop is bounded by F / 16 passes, by max_iter or by the damping's
// overflow.
// k_object_init_lite: one thread per object (a dozen products of 3-vectors).
#pragma once
#include "object_mapper_pack.hpp"   // the layout of the staged blocks
#include "object_lm_step.hpp"       // what k_object_lm uses as well: obj_lm_se3_exp, obj_lm_sym, the status codes

namespace orcvio_amd {

#define OBJ_LITE_NT 256           // threads per workgroup
#define OBJ_LITE_WPB 4            // objects (wavefronts) per workgroup

struct ObjLiteArgs {
    const ObjLmTrack* tracks;
    const double* in;
    double* out;                  // [n_tracks][OBJ_LITE_OUT]
    int n_tracks, obj_left, new_bbox, reg_every_frame, max_iter;
    double w[2], ptol;
};

struct ObjLiteInitArgs {
    ObjLmTrack* tracks;           // pad <- 1 where the optimiser must skip the object (status 4)
    double* in;                   // the staged input block; the start of every track is written
    double* out;                  // [n_tracks][OBJ_LITE_INIT_OUT]
    int n_tracks, pose_form;
    double bbox_scale[3];
};

// A (45), g (9) and c of the state x = (wTo 16 | shape 3) into S, the same in every lane.  Every lane of the wavefront calls it.
__device__ __forceinline__ void obj_lite_eval(const ObjLiteArgs& a, const int F, const double* __restrict__ blk, const double* x,
                                              const double* mean, const double wreg, double* S) {
    const int lane = (int)(threadIdx.x & 63u), t = lane & 3, grp = lane >> 2;
    ObjEvalArgs p;
    p.wTo = x; p.shape = x + 16; p.kps = nullptr;
    p.frame_wTc = blk + OBJ_LITE_O_WTC;
    p.frame_zs = nullptr;
    p.frame_bbox = p.frame_wTc + (size_t)16 * F;
    p.frame_clone = nullptr; p.frame_row0 = nullptr;
    p.K = 0; p.F = F; p.ncol = 9; p.ldhf = 9; p.rcol = -1; p.row_cols = nullptr;
    p.obj_left = a.obj_left; p.new_bbox = a.new_bbox; p.vio_left = 0; p.fix_D = 1;   // (the window columns are not used: the cheapest D)
#pragma unroll
    for (int i = 0; i < 9; ++i) p.R_b2c[i] = (i % 4 == 0) ? 1.0 : 0.0;
    p.t_c_b[0] = p.t_c_b[1] = p.t_c_b[2] = 0.0;
    p.row_clone = nullptr; p.Hx6 = nullptr; p.Hf = nullptr; p.res = nullptr;
    const double w0 = a.w[0];

#pragma unroll
    for (int i = 0; i < OBJ_LM_ACC; ++i) S[i] = 0.0;
    for (int f0 = 0; f0 < F; f0 += 16) {   // (wave-uniform bound: every lane reaches the ballot inside)
        const int f = f0 + grp;
        const bool live = f < F;
        object_rows_lane_at(p, live ? f : -1, live, t, 4,
                            [&](int, double r, const double*, const double* hpose, const double* hshape, int, const double*, int) {
            double h[9];
#pragma unroll
            for (int c = 0; c < 6; ++c) h[c] = w0 * hpose[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) h[6 + c] = w0 * hshape[c];
            const double rw = w0 * r;
            int q = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) { S[q] = fma(h[i], h[j], S[q]); ++q; }
#pragma unroll
            for (int i = 0; i < 9; ++i) S[45 + i] = fma(h[i], rw, S[45 + i]);
            S[54] = fma(rw, rw, S[54]);
        });
    }
    // over the 64 lanes, a butterfly: a + b = b + a bit for bit, so every lane ends with the same sum, in an order that depends on
    // nothing but the lane numbers
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
        for (int i = 0; i < OBJ_LM_ACC; ++i) S[i] += __shfl_xor(S[i], s);
    }
    // the regulariser without rows: wreg = w1^2 x repeats on the shape's diagonal, wreg (v - mean) in the gradient
    double reg = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = x[16 + c] - mean[c];
        S[obj_lm_sym(6 + c, 6 + c)] += wreg;
        S[45 + 6 + c] += wreg * d;
        reg = fma(wreg * d, d, reg);
    }
    S[54] += reg;
}

// (The pieces of the step are written out here and again in k_object_lm, not shared helpers: behind helpers the emitted code of one
// kernel or the other moved -- object_lm_step.hpp says which piece did what.)
__global__ __launch_bounds__(OBJ_LITE_NT) void k_object_lm_lite(ObjLiteArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int o = (int)blockIdx.x * OBJ_LITE_WPB + wave;
    if (o >= a.n_tracks) return;   // (wave-uniform; no wavefront of this kernel ever waits for another)
    const int lane = (int)(threadIdx.x & 63u);
    const ObjLmTrack tr = a.tracks[o];
    const int F = __builtin_amdgcn_readfirstlane(tr.F);
    const double* __restrict__ blk = a.in + tr.off;
    double* out = a.out + (size_t)o * OBJ_LITE_OUT;
    if (tr.pad != 0) {   // the skip word of orcvio_msckf_object_init_lm_lite: no start, no iteration -- the identity, the mean shape, status 0
        if (lane < OBJ_LITE_OUT) {
            double v = 0.0;
            if (lane < 16) v = (lane % 5 == 0) ? 1.0 : 0.0;
            else if (lane < 19) v = blk[OBJ_LITE_O_MEAN + lane - 16];
            out[lane] = v;
        }
        return;
    }
    double x[19], xn[19], mean[3], D[9];
#pragma unroll
    for (int i = 0; i < 19; ++i) x[i] = blk[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) mean[i] = blk[OBJ_LITE_O_MEAN + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) D[i] = 0.0;
    const double wreg = a.w[1] * a.w[1] * (double)(a.reg_every_frame ? F : F - 1);

    double S[OBJ_LM_ACC], Sn[OBJ_LM_ACC];
    obj_lite_eval(a, F, blk, x, mean, wreg, S);
    const double cost0 = S[54];
    int iterations = 0, evaluations = 1, status = OBJ_LM_ST_ITER_CAP;
    double lam = 1e-3;
    bool stop = false;
    if (!isfinite(cost0)) { status = OBJ_LM_ST_NONFINITE; stop = true; }

    for (int it = 0; it < a.max_iter && !stop; ++it) {
        // (A + lambda D^2) delta = -g by a Cholesky in registers: L (lower, by rows) in place of the damped matrix
        double L[9][9], dl[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
#pragma unroll
            for (int j = i; j < 9; ++j) L[j][i] = S[obj_lm_sym(i, j)];
            const double d = fmax(D[i], sqrt(S[obj_lm_sym(i, i)]));
            D[i] = d;
            L[i][i] = fma(lam * d, d, L[i][i]);
        }
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            double d = L[j][j];
#pragma unroll
            for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
            if (!(d > 0.0)) bad = true;   // (NaN included)
            const double l = sqrt(d), il = 1.0 / l;
            L[j][j] = l;
#pragma unroll
            for (int i = j + 1; i < 9; ++i) {
                double s = L[i][j];
#pragma unroll
                for (int q = 0; q < j; ++q) s -= L[i][q] * L[j][q];
                L[i][j] = s * il;
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {   // L z = -g
            double s = -S[45 + i];
#pragma unroll
            for (int q = 0; q < i; ++q) s -= L[i][q] * dl[q];
            dl[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = 8; i >= 0; --i) {  // L^T delta = z
            double s = dl[i];
#pragma unroll
            for (int q = i + 1; q < 9; ++q) s -= L[q][i] * dl[q];
            dl[i] = s / L[i][i];
        }
        // the predicted decrease, the convergence test, the trial point
        double gd = 0.0, quad = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            gd += S[45 + i] * dl[i];
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) s += S[i <= j ? obj_lm_sym(i, j) : obj_lm_sym(j, i)] * dl[j];
            quad += dl[i] * s;
        }
        const double pred = -2.0 * gd - quad;
        if (bad || !isfinite(pred)) { status = OBJ_LM_ST_NONFINITE; break; }
        if (pred <= a.ptol * S[54]) { status = OBJ_LM_ST_CONVERGED; break; }
        {
            double E[16];
            obj_lm_se3_exp(dl, E);
            const double* Lm = a.obj_left ? E : x;    // left: exp(xi) wTo, right: wTo exp(xi)
            const double* Rm = a.obj_left ? x : E;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    xn[i * 4 + j] = Lm[i * 4] * Rm[j] + Lm[i * 4 + 1] * Rm[4 + j] + Lm[i * 4 + 2] * Rm[8 + j] + Lm[i * 4 + 3] * Rm[12 + j];
#pragma unroll
            for (int i = 0; i < 3; ++i) xn[16 + i] = x[16 + i] + dl[6 + i];
        }
        obj_lite_eval(a, F, blk, xn, mean, wreg, Sn);
        ++evaluations; ++iterations;
        const double cn = Sn[54];
        if (!isfinite(cn)) { status = OBJ_LM_ST_NONFINITE; break; }
        const double rho = (S[54] - cn) / pred;
        if (rho > 1e-4) {
#pragma unroll
            for (int i = 0; i < 19; ++i) x[i] = xn[i];
#pragma unroll
            for (int i = 0; i < OBJ_LM_ACC; ++i) S[i] = Sn[i];
            const double q = 2.0 * rho - 1.0;
            lam = fmax(lam * fmax(1.0 / 3.0, 1.0 - q * q * q), 1e-12);
        } else lam *= 4.0;
        if (lam > 1e12) { status = OBJ_LM_ST_STALLED; stop = true; }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 19; ++i) out[i] = x[i];
        out[19] = cost0; out[20] = S[54];
        out[21] = (double)iterations; out[22] = (double)evaluations; out[23] = (double)status;
    }
}

__global__ __launch_bounds__(64) void k_object_init_lite(ObjLiteInitArgs a) {
    const int o = (int)(blockIdx.x * 64u + threadIdx.x);
    if (o >= a.n_tracks) return;
    const ObjLmTrack tr = a.tracks[o];
    double* blk = a.in + tr.off;
    const double* T0 = blk + OBJ_LITE_O_WTC;                          // camera -> world of frame 0: R_GtoA = R^T, p_AinG = t
    const double* bb = blk + OBJ_LITE_O_WTC + (size_t)16 * tr.F;       // frame 0's box
    double vv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { const double s = blk[OBJ_LITE_O_MEAN + i] * a.bbox_scale[i]; vv[i] = s * s; }
    const double px[4] = {bb[0], bb[2], bb[2], bb[0]}, py[4] = {bb[1], bb[1], bb[3], bb[3]};
    const double b[3] = {(bb[0] + bb[2]) / 2, (bb[1] + bb[3]) / 2, 1.0};
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int j1 = (j + 1) & 3;
        const double ln[3] = {py[j] - py[j1], px[j1] - px[j], px[j] * py[j1] - py[j] * px[j1]};   // cross((x,y,1),(x',y',1)): poly2lineh's scale
        const double lb = ln[0] * b[0] + ln[1] * b[1] + ln[2] * b[2];
        num += lb * lb;                                               // b^T (l l^T) b
#pragma unroll
        for (int i = 0; i < 3; ++i) {                                 // l^T B A B^T l with B^T l = R l
            const double y = T0[4 * i] * ln[0] + T0[4 * i + 1] * ln[1] + T0[4 * i + 2] * ln[2];
            den += vv[i] * y * y;
        }
    }
    const double d = 1.0 / sqrt(num / den);
    double wPq[3];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        wPq[i] = d * (T0[4 * i] * b[0] + T0[4 * i + 1] * b[1] + T0[4 * i + 2] * b[2]) + T0[4 * i + 3];   // d B^T b + p_AinG
        finite = finite && isfinite(wPq[i]);
    }
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (finite) {
        T[3] = wPq[0]; T[7] = wPq[1];
        if (a.pose_form == 0) T[11] = wPq[2];   // forms 1 and 2: poseSE32SE2 of an identity rotation -- yaw 0, translation (x, y, 0)
    }
    double* out = a.out + (size_t)o * OBJ_LITE_INIT_OUT;
#pragma unroll
    for (int i = 0; i < 16; ++i) { out[i] = T[i]; blk[i] = T[i]; }
    out[16] = d;
    out[17] = finite ? 1.0 : 4.0;
    // the rest of the optimiser's start: the mean shape (the reference's LMObjectStateLite)
#pragma unroll
    for (int i = 0; i < 3; ++i) blk[16 + i] = blk[OBJ_LITE_O_MEAN + i];
    a.tracks[o].pad = finite ? 0 : 1;
}

}  // namespace orcvio_amd

// object_lm.hpp -- the object optimiser on the device: batched Levenberg-Marquardt over the object state
// x = (wTo in SE(3), shape v, keypoints m_k), 9 + 3K degrees of freedom in the column order [pose 6 | shape 3 | 3 per keypoint].
// Reference: ObjectFeatureInitializer::single_levenberg_marquardt (src/obj/ObjectFeatureInitializer.cpp:346-440) over the ObjectLM
// functor (src/obj/ObjectLM.cpp:761-816): w0 keypoint rows, w1 bbox rows, w2 (m_k - mean_k) and w3 (v - mean_v) repeated once per
// frame (:652-684, :732-743), Huber off.  The reference's Eigen LM carries a custom scaled_norm, so its trajectory is not
// reproduced: the iteration is the one documented in include/orcvio_msckf.h, and the optimum is what is comparable.
//
// One workgroup per object, the whole iteration inside the launch; no workgroup waits for another, the loop is bounded by max_iter
// and by the damping's overflow.  The rows are never materialised: the lanes stride over the frames (64 / lpf frames per wavefront
// side by side, object_rows_lane_at -- the same body k_object_rows and k_obj_fused evaluate), and each lane keeps the normal
// equations of its OWN role: a keypoint lane touches the pose and its keypoint, a bbox lane the pose and the shape, so nine columns
// (45 products, 9 gradient entries, the cost) per lane hold everything.  A = J^T J is an arrow -- a dense 9 x 9 head, K independent
// 3 x 3 blocks, 6 x 3 couplings -- and stays one with the damping added: the blocks are eliminated by a Schur complement, the head
// is factored by a 9 x 9 Cholesky, the blocks are back-substituted.  The two regularisers add w^2 F to the diagonal and
// w^2 F (x - mean) to the gradient: they need no rows.
#pragma once
#include "object_mapper_pack.hpp"   // ObjLmTrack, the limits, the layout of the staged blocks
#include "object_lm_step.hpp"       // what k_object_lm_lite uses as well: obj_lm_se3_exp, obj_lm_sym, the status codes

namespace orcvio_amd {

#define OBJ_LM_NT 256           // threads per workgroup (four wavefronts)
#define OBJ_LM_STATE 68         // wTo 16 | shape 3 | kps 48 (| 1 unused)

struct ObjLmArgs {
    const ObjLmTrack* tracks;
    const double* in;
    double* out;                // [n_tracks][OBJ_LM_OUT]
    int obj_left, new_bbox, max_iter;
    double w[4], ptol;
};

// the assembled normal equations of one state
struct ObjLmSys {
    double H[81];               // head: pose and shape, full symmetric
    double g[9];
    double Akk[OBJ_LM_MAXK][6]; // xx xy xz yy yz zz
    double Apk[OBJ_LM_MAXK][18];// pose (6) x keypoint (3), row-major
    double gk[OBJ_LM_MAXK][3];
    double c;
};

// A, g and c of the state at `x` (LDS) into `S` (LDS).  Every thread of the workgroup calls it; it ends behind a barrier.
__device__ __forceinline__ void obj_lm_eval(const ObjLmArgs& a, const ObjLmTrack tr, const double* __restrict__ in, const double* x,
                                            const double* prior, double (*sRole)[OBJ_LM_ACC + 1], ObjLmSys* S) {
    const int K = tr.K, F = tr.F;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lpf = K + 4 <= 8 ? 8 : (K + 4 <= 16 ? 16 : 32);
    const int fpw = 64 / lpf, t = lane % lpf, grp = lane / lpf;
    ObjEvalArgs p;
    p.wTo = x; p.shape = x + 16; p.kps = x + 19;
    p.frame_wTc = in + tr.off + 22 + 6 * K;
    p.frame_zs = p.frame_wTc + (size_t)16 * F;
    p.frame_bbox = p.frame_zs + (size_t)2 * K * F;
    p.frame_clone = nullptr; p.frame_row0 = nullptr;
    p.K = K; p.F = F; p.ncol = 9 + 3 * K; p.ldhf = p.ncol; p.rcol = -1; p.row_cols = nullptr;
    p.obj_left = a.obj_left; p.new_bbox = a.new_bbox; p.vio_left = 0; p.fix_D = 1;   // (the window columns are not used: the cheapest D)
    for (int i = 0; i < 9; ++i) p.R_b2c[i] = (i % 4 == 0) ? 1.0 : 0.0;
    p.t_c_b[0] = p.t_c_b[1] = p.t_c_b[2] = 0.0;
    p.row_clone = nullptr; p.Hx6 = nullptr; p.Hf = nullptr; p.res = nullptr;
    const double w0 = a.w[0], w1 = a.w[1];

    double acc[OBJ_LM_ACC];
#pragma unroll
    for (int i = 0; i < OBJ_LM_ACC; ++i) acc[i] = 0.0;
    for (int f0 = 0; f0 < F; f0 += (OBJ_LM_NT / 64) * fpw) {   // (workgroup-uniform bound: every lane reaches the ballot inside)
        const int f = f0 + wave * fpw + grp;
        const bool live = f < F;
        object_rows_lane_at(p, live ? f : -1, live, t, lpf,
                            [&](int, double r, const double*, const double* hpose, const double* hshape, int, const double* hkp, int) {
            const double w = hshape ? w1 : w0;
            const double* tail = hshape ? hshape : hkp;
            double h[9];
#pragma unroll
            for (int c = 0; c < 6; ++c) h[c] = w * hpose[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) h[6 + c] = w * tail[c];
            const double rw = w * r;
            int q = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) { acc[q] = fma(h[i], h[j], acc[q]); ++q; }
#pragma unroll
            for (int i = 0; i < 9; ++i) acc[45 + i] = fma(h[i], rw, acc[45 + i]);
            acc[54] = fma(rw, rw, acc[54]);
        });
    }
    // lanes of one role: over the frame groups of the wavefront (butterfly: every lane ends with the same sum) ...
    for (int s = lpf; s < 64; s <<= 1) {
#pragma unroll
        for (int i = 0; i < OBJ_LM_ACC; ++i) acc[i] += __shfl_xor(acc[i], s);
    }
    // ... and over the wavefronts in LDS, in wave order (the same order whatever else the launch holds: a batch and a single call agree bit for bit)
    for (int w = 0; w < OBJ_LM_NT / 64; ++w) {
        if (wave == w && grp == 0 && t < K + 4) {
#pragma unroll
            for (int i = 0; i < OBJ_LM_ACC; ++i) sRole[t][i] = (w == 0 ? 0.0 : sRole[t][i]) + acc[i];
        }
        __syncthreads();
    }
    // assembly: the head by threads 0..54 (one entry each, roles summed in order), the keypoint blocks by threads 64..64+K-1
    const double* mean_shape = prior;
    const double* mean_kps = prior + 3;
    const double w2F = a.w[2] * a.w[2] * (double)F, w3F = a.w[3] * a.w[3] * (double)F;
    if (tid < OBJ_LM_ACC) {
        int i = 0, j = 0;         // entry tid: product (i, j), gradient entry i (j = -1), or the cost (i = -1)
        if (tid < 45) { int q = tid; while (q >= 9 - i) { q -= 9 - i; ++i; } j = i + q; }
        else if (tid < 54) { i = tid - 45; j = -1; }
        else { i = -1; j = -1; }
        const bool tail = i >= 6 || j >= 6;   // shape columns: the bbox lanes only (a keypoint lane's tail is its keypoint)
        double s = 0.0;
        for (int r = tail ? K : 0; r < K + 4; ++r) s += sRole[r][tid];
        if (tid < 45) {
            if (i == j && i >= 6) s += w3F;
            S->H[i * 9 + j] = s; S->H[j * 9 + i] = s;
        } else if (tid < 54) {
            if (i >= 6) s += w3F * (x[16 + i - 6] - mean_shape[i - 6]);
            S->g[i] = s;
        } else {
            double reg = 0.0;
            for (int c = 0; c < 3; ++c) { const double d = x[16 + c] - mean_shape[c]; reg = fma(w3F * d, d, reg); }
            for (int c = 0; c < 3 * K; ++c) { const double d = x[19 + c] - mean_kps[c]; reg = fma(w2F * d, d, reg); }
            S->c = s + reg;
        }
    } else if (tid >= 64 && tid < 64 + K) {
        const int k = tid - 64;
        int q = 0;
        for (int aa = 0; aa < 3; ++aa)
            for (int bb = aa; bb < 3; ++bb) S->Akk[k][q++] = sRole[k][obj_lm_sym(6 + aa, 6 + bb)] + (aa == bb ? w2F : 0.0);
        for (int i = 0; i < 6; ++i)
            for (int bb = 0; bb < 3; ++bb) S->Apk[k][i * 3 + bb] = sRole[k][obj_lm_sym(i, 6 + bb)];
        for (int bb = 0; bb < 3; ++bb) S->gk[k][bb] = sRole[k][45 + 6 + bb] + w2F * (x[19 + 3 * k + bb] - mean_kps[3 * k + bb]);
    }
    __syncthreads();
}

// (The pieces of the step are written out here and again in k_object_lm_lite, not shared helpers: behind helpers the emitted code of
// one kernel or the other moved -- object_lm_step.hpp says which piece did what.)
__global__ __launch_bounds__(OBJ_LM_NT) void k_object_lm(ObjLmArgs a) {
    __shared__ double sX[2][OBJ_LM_STATE];            // the accepted state and the trial state
    __shared__ double sPrior[3 + 3 * OBJ_LM_MAXK];    // mean shape | mean keypoints
    __shared__ double sRole[OBJ_LM_MAXK + 4][OBJ_LM_ACC + 1];
    __shared__ ObjLmSys sS[2];
    __shared__ double sD[9 + 3 * OBJ_LM_MAXK];        // the scaling: largest sqrt(A_jj) so far
    __shared__ double sW[OBJ_LM_MAXK][18], sY[OBJ_LM_MAXK][3], sC[OBJ_LM_MAXK][42], sQ[OBJ_LM_MAXK][2];
    __shared__ double sDelta[9 + 3 * OBJ_LM_MAXK];
    __shared__ double sLam;
    __shared__ int sCtl[4];                            // stop | accept | status | bad pivot

    const int o = (int)blockIdx.x, tid = (int)threadIdx.x;
    const ObjLmTrack tr = a.tracks[o];
    const int K = tr.K;
    const double* __restrict__ in = a.in;
    if (tr.pad != 0) {   // the skip word of orcvio_msckf_object_init_lm: no start, no iteration -- the identity, the means, status 0
        double* out = a.out + (size_t)o * OBJ_LM_OUT;
        for (int i = tid; i < OBJ_LM_OUT; i += OBJ_LM_NT) {
            double v = 0.0;
            if (i < 16) v = (i % 5 == 0) ? 1.0 : 0.0;
            else if (i < 19 + 3 * K) v = in[tr.off + 3 + 3 * K + i];
            out[i] = v;
        }
        return;          // (workgroup-uniform)
    }
    for (int i = tid; i < OBJ_LM_STATE; i += OBJ_LM_NT) {
        double v = 0.0;
        if (i < 16) v = in[tr.off + i];
        else if (i < 19 + 3 * K) v = in[tr.off + i];
        sX[0][i] = v; sX[1][i] = v;
    }
    for (int i = tid; i < 3 + 3 * OBJ_LM_MAXK; i += OBJ_LM_NT) sPrior[i] = i < 3 + 3 * K ? in[tr.off + 19 + 3 * K + i] : 0.0;
    for (int i = tid; i < 9 + 3 * OBJ_LM_MAXK; i += OBJ_LM_NT) { sD[i] = 0.0; sDelta[i] = 0.0; }
    if (tid == 0) { sLam = 1e-3; sCtl[0] = 0; sCtl[1] = 0; sCtl[2] = OBJ_LM_ST_ITER_CAP; sCtl[3] = 0; }
    __syncthreads();

    int cur = 0, iterations = 0, evaluations = 1;
    obj_lm_eval(a, tr, in, sX[0], sPrior, sRole, &sS[0]);
    const double cost0 = sS[0].c;
    if (!isfinite(cost0)) { if (tid == 0) { sCtl[2] = OBJ_LM_ST_NONFINITE; sCtl[0] = 1; } }
    __syncthreads();
    bool stop = sCtl[0] != 0;

    for (int it = 0; it < a.max_iter && !stop; ++it) {
        const ObjLmSys* S = &sS[cur];
        const double* x = sX[cur];
        double* xn = sX[cur ^ 1];
        // A: the keypoint blocks -- B_k = (A_kk + lambda D_k^2)^-1 by a 3 x 3 Cholesky, W_k = A_pk B_k, y_k = B_k g_k, and what the
        // block takes out of the head: C_k = W_k A_pk^T, A_pk y_k
        if (tid < K) {
            const int k = tid;
            const double lam = sLam;
            double m[6];
            for (int q = 0; q < 6; ++q) m[q] = S->Akk[k][q];
            const int dq[3] = {0, 3, 5};
            for (int c = 0; c < 3; ++c) {
                const double d = fmax(sD[9 + 3 * k + c], sqrt(m[dq[c]]));
                sD[9 + 3 * k + c] = d;
                m[dq[c]] = fma(lam * d, d, m[dq[c]]);
            }
            // M = L L^T; B = M^-1 = L^-T L^-1
            const double l00 = sqrt(m[0]), i00 = 1.0 / l00;
            const double l10 = m[1] * i00, l20 = m[2] * i00;
            const double d1 = m[3] - l10 * l10;
            const double l11 = sqrt(d1), i11 = 1.0 / l11;
            const double l21 = (m[4] - l20 * l10) * i11;
            const double d2 = m[5] - l20 * l20 - l21 * l21;
            const double l22 = sqrt(d2), i22 = 1.0 / l22;
            if (!(m[0] > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) sCtl[3] = 1;   // (NaN included; benign race: every writer stores 1)
            // Li = L^-1 (lower)
            const double a10 = -l10 * i00 * i11, a20 = (-l20 * i00 - l21 * a10) * i22, a21 = -l21 * i11 * i22;
            double B[9];
            B[0] = i00 * i00 + a10 * a10 + a20 * a20; B[1] = a10 * i11 + a20 * a21; B[2] = a20 * i22;
            B[4] = i11 * i11 + a21 * a21; B[5] = a21 * i22; B[8] = i22 * i22;
            B[3] = B[1]; B[6] = B[2]; B[7] = B[5];
            double W[18], y[3];
            for (int i = 0; i < 6; ++i)
                for (int c = 0; c < 3; ++c) {
                    W[i * 3 + c] = S->Apk[k][i * 3] * B[c] + S->Apk[k][i * 3 + 1] * B[3 + c] + S->Apk[k][i * 3 + 2] * B[6 + c];
                    sW[k][i * 3 + c] = W[i * 3 + c];
                }
            for (int c = 0; c < 3; ++c) { y[c] = B[c * 3] * S->gk[k][0] + B[c * 3 + 1] * S->gk[k][1] + B[c * 3 + 2] * S->gk[k][2]; sY[k][c] = y[c]; }
            for (int i = 0; i < 6; ++i) {
                for (int j = 0; j < 6; ++j)
                    sC[k][i * 6 + j] = W[i * 3] * S->Apk[k][j * 3] + W[i * 3 + 1] * S->Apk[k][j * 3 + 1] + W[i * 3 + 2] * S->Apk[k][j * 3 + 2];
                sC[k][36 + i] = S->Apk[k][i * 3] * y[0] + S->Apk[k][i * 3 + 1] * y[1] + S->Apk[k][i * 3 + 2] * y[2];
            }
        }
        __syncthreads();
        // B: the head -- (H + lambda D^2 - sum_k C_k) delta_h = -(g_h - sum_k A_pk y_k) by a 9 x 9 Cholesky
        if (tid == 0) {
            const double lam = sLam;
            double M[81], rhs[9];
            for (int i = 0; i < 81; ++i) M[i] = S->H[i];
            for (int i = 0; i < 9; ++i) {
                const double d = fmax(sD[i], sqrt(S->H[i * 9 + i]));
                sD[i] = d;
                M[i * 9 + i] = fma(lam * d, d, M[i * 9 + i]);
                rhs[i] = S->g[i];
            }
            for (int k = 0; k < K; ++k) {
                for (int i = 0; i < 6; ++i) {
                    for (int j = 0; j < 6; ++j) M[i * 9 + j] -= 0.5 * (sC[k][i * 6 + j] + sC[k][j * 6 + i]);
                    rhs[i] -= sC[k][36 + i];
                }
            }
            bool bad = sCtl[3] != 0;
            for (int j = 0; j < 9; ++j) {   // M = L L^T in place (lower)
                double d = M[j * 9 + j];
                for (int q = 0; q < j; ++q) d -= M[j * 9 + q] * M[j * 9 + q];
                if (!(d > 0.0)) bad = true;
                const double l = sqrt(d), il = 1.0 / l;
                M[j * 9 + j] = l;
                for (int i = j + 1; i < 9; ++i) {
                    double s = M[i * 9 + j];
                    for (int q = 0; q < j; ++q) s -= M[i * 9 + q] * M[j * 9 + q];
                    M[i * 9 + j] = s * il;
                }
            }
            for (int i = 0; i < 9; ++i) {   // L z = -rhs
                double s = -rhs[i];
                for (int q = 0; q < i; ++q) s -= M[i * 9 + q] * rhs[q];
                rhs[i] = s / M[i * 9 + i];
            }
            for (int i = 8; i >= 0; --i) {  // L^T delta = z
                double s = rhs[i];
                for (int q = i + 1; q < 9; ++q) s -= M[q * 9 + i] * rhs[q];
                rhs[i] = s / M[i * 9 + i];
            }
            for (int i = 0; i < 9; ++i) sDelta[i] = rhs[i];
            sCtl[3] = bad ? 1 : 0;
        }
        __syncthreads();
        // C: back-substitution delta_k = -y_k - W_k^T delta_p, and the block's share of g^T delta and delta^T A delta
        if (tid < K) {
            const int k = tid;
            double dk[3];
            for (int c = 0; c < 3; ++c) {
                double s = -sY[k][c];
                for (int i = 0; i < 6; ++i) s -= sW[k][i * 3 + c] * sDelta[i];
                dk[c] = s; sDelta[9 + 3 * k + c] = s;
            }
            const double* A = S->Akk[k];
            double quad = A[0] * dk[0] * dk[0] + A[3] * dk[1] * dk[1] + A[5] * dk[2] * dk[2] +
                          2.0 * (A[1] * dk[0] * dk[1] + A[2] * dk[0] * dk[2] + A[4] * dk[1] * dk[2]);
            for (int i = 0; i < 6; ++i)
                quad += 2.0 * sDelta[i] * (S->Apk[k][i * 3] * dk[0] + S->Apk[k][i * 3 + 1] * dk[1] + S->Apk[k][i * 3 + 2] * dk[2]);
            sQ[k][0] = S->gk[k][0] * dk[0] + S->gk[k][1] * dk[1] + S->gk[k][2] * dk[2];
            sQ[k][1] = quad;
        }
        __syncthreads();
        // D: the predicted decrease, the convergence test, the trial point
        if (tid == 0) {
            double gd = 0.0, quad = 0.0;
            for (int i = 0; i < 9; ++i) {
                gd += S->g[i] * sDelta[i];
                double s = 0.0;
                for (int j = 0; j < 9; ++j) s += S->H[i * 9 + j] * sDelta[j];
                quad += sDelta[i] * s;
            }
            for (int k = 0; k < K; ++k) { gd += sQ[k][0]; quad += sQ[k][1]; }
            const double pred = -2.0 * gd - quad;
            sQ[0][0] = pred;
            if (sCtl[3] != 0 || !isfinite(pred)) { sCtl[2] = OBJ_LM_ST_NONFINITE; sCtl[0] = 1; }
            else if (pred <= a.ptol * S->c) { sCtl[2] = OBJ_LM_ST_CONVERGED; sCtl[0] = 1; }
            else {
                double E[16];
                obj_lm_se3_exp(sDelta, E);
                const double* L = a.obj_left ? E : x;    // left: exp(xi) wTo, right: wTo exp(xi)
                const double* R = a.obj_left ? x : E;
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j)
                        xn[i * 4 + j] = L[i * 4] * R[j] + L[i * 4 + 1] * R[4 + j] + L[i * 4 + 2] * R[8 + j] + L[i * 4 + 3] * R[12 + j];
                for (int i = 0; i < 3 + 3 * K; ++i) xn[16 + i] = x[16 + i] + sDelta[6 + i];
            }
        }
        __syncthreads();
        if (sCtl[0] != 0) break;   // (workgroup-uniform)
        const double pred = sQ[0][0];
        obj_lm_eval(a, tr, in, xn, sPrior, sRole, &sS[cur ^ 1]);
        ++evaluations; ++iterations;
        if (tid == 0) {
            const double c = S->c, cn = sS[cur ^ 1].c;
            double lam = sLam;
            sCtl[1] = 0;
            if (!isfinite(cn)) { sCtl[2] = OBJ_LM_ST_NONFINITE; sCtl[0] = 1; }
            else {
                const double rho = (c - cn) / pred;
                if (rho > 1e-4) {
                    sCtl[1] = 1;
                    const double q = 2.0 * rho - 1.0;
                    lam = fmax(lam * fmax(1.0 / 3.0, 1.0 - q * q * q), 1e-12);
                } else lam *= 4.0;
                if (lam > 1e12) { sCtl[2] = OBJ_LM_ST_STALLED; sCtl[0] = 1; }
                sLam = lam;
            }
        }
        __syncthreads();
        if (sCtl[1] != 0) cur ^= 1;
        stop = sCtl[0] != 0;
        __syncthreads();           // (thread 0 writes the control words again in the next step)
    }
    double* out = a.out + (size_t)o * OBJ_LM_OUT;
    for (int i = tid; i < 67; i += OBJ_LM_NT) out[i] = sX[cur][i];
    if (tid == 0) {
        out[67] = cost0; out[68] = sS[cur].c;
        out[69] = (double)iterations; out[70] = (double)evaluations; out[71] = (double)sCtl[2];
    }
}

}  // namespace orcvio_amd

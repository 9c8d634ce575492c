// Batched full-mesh LBS, float32 out: verts[F][V][3] for F frames of pose variables.
// Replaces SmplModelLBS.r (src/moshpp/models/smpl_fast_derivatives.py:206-218,243-244 -> psbody verts_decorated)
// evaluated for a whole solved sequence at once (mesh export of a Stage-II result).
//
// Per (vertex, frame) the work is 2*3*9(K-1) flop of pose correctives (SMPL-H: 2754) against 12 bytes of output, i.e.
// 230 flop/B: on the f32 pipes (157 TF) that is 19x above the HBM ridge, on the f16 matrix pipes (2.5 PF) it sits AT the
// ridge.  So the corrective contraction  C[v,i,f] = sum_q posedirs[v,i,q] * (R - I)[f,q]  runs on
// v_mfma_f32_16x16x32_f16 (f16 operands, scaled so posedirs stay in the normal range; f32 accumulate), and everything
// else is fused behind it so that HBM sees the 12 V F output bytes once.
//
//   k_lbs_prep   one wavefront per frame: hand-PCA -> fullpose, Rodrigues, kinematic chain; writes the skinning transforms
//                Atr[16-frame block][joint][frame][12] (f32, translation folded with trans[f]) -- one contiguous K x 768 B
//                block per 16 frames, from which the export kernel's waves gather their joints -- and the pose features as MFMA B fragments
//                featF[128-frame tile][k-step][16-frame block][lane][8] (f16).
//   k_lbs_export two persistent workgroups per CU (4 waves each), a tile = 64 vertices x 128 frames, a wave = 16 vertices x 128
//                frames = 8 MFMA tiles of 16 x 16 per coordinate (96 accumulator registers); k-loop with the features through a
//                three-slot LDS ring, blend over per-group joint lists with packed FMAs, rows out through an LDS exchange --
//                described at the kernel.  (Rounds 3/4: k_lbs_tile, one workgroup of eight waves per CU, 128 x 128 tiles, a
//                per-vertex four-influence gather from LDS: 216 us per 4000-frame SMPL-H export, 0.18 of the HBM peak.)
//
// Accuracy: f16 operands give |err| ~ 2^-11 |posedirs| |R - I| sqrt(9(K-1)) ~ 5e-6 m for millimetre-scale correctives
// (tests bound it at 2e-5 m); moshii_lbs_forward_f64 is the reference-precision path.
//
// Free shape block (moshii_lbs_forward_shape_f32: per-frame expression / DMPL coefficients c_f, template parameter SH of the three
// kernels; SH = false is the code without): v_posed gains S_free . c_f as KSX = ceil(3 nshape / 32) k-steps IN FRONT of the pose
// k-steps -- every coefficient three columns, d_hi c_hi + d_hi c_lo + d_lo c_hi with (hi, lo) f16 pairs of direction and coefficient and a
// power-of-two scale of their own (directions x pscale / sxscale, largest at 2^7 .. 2^8; coefficients x sxscale) -- and k_lbs_prep
// moves the joints, J_f = J + JS . c_f in f32, ahead of the chain.  Measured on the MI355X against the oracle, every vertex of every
// frame: 6.1e-6 m (SMPL-X, 80 coefficients), 6.7e-6 m (SMPL-H, 8), 3.8e-6 m (SMPL, 125) -- the pose features' error, as without a
// block; SMPL-X with 80 coefficients 386 us per 4000-frame export against 303 us without (profiles/lbs_shape_export.txt).
#include "../../include/moshii.h"
#include "moshii_dev.h"
#include "dev_mem.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte, dword-aligned store unit
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

extern "C" {
int moshii_internal_model_dims(moshii_model_t m, int* V, int* K);
const double* moshii_internal_vsh(moshii_model_t m);
const double* moshii_internal_posedirs(moshii_model_t m);
const double* moshii_internal_weights(moshii_model_t m);
const double* moshii_internal_J(moshii_model_t m);
const double* moshii_internal_weights_host(moshii_model_t m);
const double* moshii_internal_shape_block(moshii_model_t m, int* NB, int* start, int* count, const double** JS);
void* moshii_internal_l32(moshii_model_t m);
void moshii_internal_l32_set_valid(moshii_model_t m, int v);
}

namespace {

__global__ void k_cvt_vsh(int n, const double* __restrict__ src, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

__global__ void k_cvt_posedirs(int V, int Vp, int nfeat, const double* __restrict__ src, float* __restrict__ dst) {
    // dst[(q*3 + i)*Vp + v] = src[(v*3 + i)*nfeat + q]
    const size_t total = (size_t)nfeat * 3 * Vp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int v = (int)(idx % Vp);
        const int qi = (int)(idx / Vp);
        const int q = qi / 3, i = qi % 3;
        dst[idx] = (v < V) ? (float)src[((size_t)v * 3 + i) * nfeat + q] : 0.0f;
    }
}

__global__ void k_cvt_weights(int V, int Vp, int K, const double* __restrict__ src, float* __restrict__ dst) {
    const size_t total = (size_t)K * Vp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int v = (int)(idx % Vp);
        const int j = (int)(idx / Vp);
        dst[idx] = (v < V) ? (float)src[(size_t)v * K + j] : 0.0f;
    }
}

// max |posedirs| (for the f16 scale)
__global__ void k_absmax(size_t n, const double* __restrict__ src, double* __restrict__ out) {
    __shared__ double red[256];
    double m = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmax(m, fabs(src[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// fragment-major f16 posedirs (MFMA A operand of v_mfma_f32_16x16x32_f16): record (group, i, ks) holds, for lane l, the 8 values
// posedirs[v = perm[16 group + (l & 15)]][i][32 ks + 8 (l >> 4) + e]  (perm: the export kernel's vertex groups, -1 = padding)
__global__ void k_pack_pfrag(int nfeat, int KS, int ng, double pscale, const int* __restrict__ perm, const double* __restrict__ src, _Float16* __restrict__ dst) {
    const size_t total = (size_t)ng * 3 * KS * 64 * 8;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 7);
        const int l = (int)((idx >> 3) & 63);
        size_t r = idx >> 9;
        const int ks = (int)(r % KS); r /= KS;
        const int i = (int)(r % 3);
        const int g = (int)(r / 3);
        const int v = perm[g * 16 + (l & 15)];
        const int q = ks * 32 + (l >> 4) * 8 + e;
        double val = 0.0;
        if (v >= 0 && q < nfeat) val = src[((size_t)v * 3 + i) * nfeat + q] * pscale;
        dst[idx] = (_Float16)val;
    }
}

// ---- free shape block (moshii_lbs_forward_shape_f32) ----
// The block's fragments IN FRONT of the pose fragments: record (group, i, ks) of PfragX, KST = KSX + KS k-steps a row.  k-steps
// ks < KSX hold the shape columns q = 32 ks + 8 (l >> 4) + e: coefficient q / 3, part q % 3 -- parts 0 and 1 the f16 HIGH half of
// shapedirs[v][i][start + q / 3] * scale (against the coefficient's high and low half), part 2 the LOW half (the residual of the
// high one, against the coefficient's high half); scale = pscale / sxscale.  k-steps behind them: a copy of Pfrag's.
__global__ void k_pack_pfrag_shape(int NB, int start, int E, int KSX, int KS, int ng, double scale, const int* __restrict__ perm,
                                   const double* __restrict__ sd, const _Float16* __restrict__ pfrag, _Float16* __restrict__ dst) {
    const int KST = KSX + KS;
    const size_t total = (size_t)ng * 3 * KST * 64 * 8;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 7);
        const int l = (int)((idx >> 3) & 63);
        size_t r = idx >> 9;
        const int ks = (int)(r % KST); r /= KST;
        const int i = (int)(r % 3);
        const int g = (int)(r / 3);
        if (ks >= KSX) { dst[idx] = pfrag[((((size_t)g * 3 + i) * KS + (ks - KSX)) * 64 + l) * 8 + e]; continue; }
        const int v = perm[g * 16 + (l & 15)];
        const int q = ks * 32 + (l >> 4) * 8 + e, c = q / 3, part = q - 3 * c;
        _Float16 val = (_Float16)0.0f;
        if (v >= 0 && c < E) {
            const double d = sd[((size_t)v * 3 + i) * NB + start + c] * scale;
            const _Float16 hi = (_Float16)d;
            val = part < 2 ? hi : (_Float16)(d - (double)hi);
        }
        dst[idx] = val;
    }
}

// JSf[(k E + e)][4] = {JS[k][e][0..2], 0} (f32): one 16-byte load per (joint, coefficient) in k_lbs_prep
__global__ void k_cvt_js(int n, const double* __restrict__ JS, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 3; ++c) dst[i * 4 + c] = (float)JS[(size_t)i * 3 + c];
    dst[i * 4 + 3] = 0.0f;
}

// Sft[(e*3 + i)*Vp + v] = shapedirs[v][i][start + e]  (plain kernel)
__global__ void k_cvt_shapedirs(int V, int Vp, int NB, int start, int E, const double* __restrict__ sd, float* __restrict__ dst) {
    const size_t total = (size_t)E * 3 * Vp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int v = (int)(idx % Vp);
        const int ei = (int)(idx / Vp);
        dst[idx] = (v < V) ? (float)sd[((size_t)v * 3 + ei % 3) * NB + start + ei / 3] : 0.0f;
    }
}

// max |shapedirs[:, :, start : start + E]|
__global__ void k_absmax_block(size_t rows, int NB, int start, int E, const double* __restrict__ src, double* __restrict__ out) {
    __shared__ double red[256];
    double m = 0.0;
    const size_t n = rows * (size_t)E;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmax(m, fabs(src[(i / E) * NB + start + i % E]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// rest positions in group order, x pscale: vshs[slot] = {x, y, z, 0} of vertex perm[slot]
__global__ void k_pack_vsh(int n, float pscale, const int* __restrict__ perm, const double* __restrict__ vsh, float* __restrict__ dst) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int v = perm[s];
    for (int c = 0; c < 3; ++c) dst[s * 4 + c] = v >= 0 ? (float)(vsh[(size_t)v * 3 + c] * (double)pscale) : 0.0f;
    dst[s * 4 + 3] = 0.0f;
}

// ---- fallback kernel: one workgroup = 256 vertices of one frame (plain f32, dense weights) ----------------
// shape: rows of free-shape coefficients [F][lm.nshape], or null -- the frame's joints then move by JS . shape[f] (LDS copy Jf), its
// rest positions by the block's directions
__global__ __launch_bounds__(256) void k_lbs_f32_v0(ModelDev md, Lbs32Model lm, const float* __restrict__ pose,
                                                     const float* __restrict__ trans, const float* __restrict__ shape, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    const int K = md.K, P = md.P;
    float* fullpose = smf;            // P
    float* Rl = fullpose + P;         // K*9
    float* A = Rl + K * 9;            // K*12 : [Rw | tw - Rw J]
    float* feat = A + K * 12;         // K*9
    float* Jf = feat + K * 9;         // K*3: this frame's joints
    const int f = blockIdx.y, tid = threadIdx.x;
    const int E = shape != nullptr ? lm.nshape : 0;
    const float* cf = shape != nullptr ? shape + (size_t)f * E : nullptr;
    for (int d = tid; d < K * 3; d += blockDim.x) {
        float s = lm.J[d];
        for (int e = 0; e < E; ++e) s = fmaf(lm.JSf[((size_t)(d / 3) * E + e) * 4 + d % 3], cf[e], s);
        Jf[d] = s;
    }
    const float* ps = pose + (size_t)f * md.NP;
    for (int d = tid; d < P; d += blockDim.x) {
        float v;
        if (d < md.body_dof) v = ps[d];
        else {
            const int h = d - md.body_dof;
            double acc = md.hands_mean[h];
            for (int i = 0; i < md.hand_dof; ++i) acc += (double)ps[md.body_dof + i] * md.comps[i * md.nhand_full + h];
            v = (float)acc;
        }
        fullpose[d] = v;
    }
    __syncthreads();
    if (tid < K) {
        const float x = fullpose[3 * tid], y = fullpose[3 * tid + 1], z = fullpose[3 * tid + 2];
        const float t2 = x * x + y * y + z * z;
        float a, b;
        if (t2 < 1e-6f) { a = 1.0f - t2 / 6.0f; b = 0.5f - t2 / 24.0f; }
        else { const float t = sqrtf(t2); a = sinf(t) / t; b = (1.0f - cosf(t)) / t2; }
        const float K2[9] = {x * x - t2, x * y, x * z, x * y, y * y - t2, y * z, x * z, y * z, z * z - t2};
        const float Km[9] = {0.0f, -z, y, z, 0.0f, -x, -y, x, 0.0f};
        for (int e = 0; e < 9; ++e) {
            const float id = (e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f;
            const float r = id + a * Km[e] + b * K2[e];
            Rl[tid * 9 + e] = r;
            feat[tid * 9 + e] = r - id;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float Rw[MOSHII_MAXK * 9], tw[MOSHII_MAXK * 3];
        for (int e = 0; e < 9; ++e) Rw[e] = Rl[e];
        for (int i = 0; i < 3; ++i) tw[i] = Jf[i];
        for (int k = 1; k < K; ++k) {
            const int p = md.parents[k];
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j)
                    Rw[k * 9 + i * 3 + j] = Rw[p * 9 + i * 3 + 0] * Rl[k * 9 + j] + Rw[p * 9 + i * 3 + 1] * Rl[k * 9 + 3 + j] + Rw[p * 9 + i * 3 + 2] * Rl[k * 9 + 6 + j];
                tw[k * 3 + i] = Rw[p * 9 + i * 3 + 0] * (Jf[k * 3 + 0] - Jf[p * 3 + 0]) + Rw[p * 9 + i * 3 + 1] * (Jf[k * 3 + 1] - Jf[p * 3 + 1]) +
                                Rw[p * 9 + i * 3 + 2] * (Jf[k * 3 + 2] - Jf[p * 3 + 2]) + tw[p * 3 + i];
            }
        }
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) A[k * 12 + i * 4 + j] = Rw[k * 9 + i * 3 + j];
                A[k * 12 + i * 4 + 3] = tw[k * 3 + i] - (Rw[k * 9 + i * 3 + 0] * Jf[k * 3 + 0] + Rw[k * 9 + i * 3 + 1] * Jf[k * 3 + 1] + Rw[k * 9 + i * 3 + 2] * Jf[k * 3 + 2]);
            }
    }
    __syncthreads();
    const int v = blockIdx.x * blockDim.x + tid;
    if (v >= md.V) return;
    const int nfeat = 9 * (K - 1), Vp = lm.Vp;
    float vp[3] = {lm.v_shaped[v * 3 + 0], lm.v_shaped[v * 3 + 1], lm.v_shaped[v * 3 + 2]};
    for (int q = 0; q < nfeat; ++q) {
        const float fq = feat[9 + q];
        const float* pq = lm.posedirs_t + (size_t)q * 3 * Vp + v;
        vp[0] += pq[0] * fq; vp[1] += pq[Vp] * fq; vp[2] += pq[2 * Vp] * fq;
    }
    for (int e = 0; e < E; ++e) {
        const float ce = cf[e];
        const float* sq = lm.Sft + (size_t)e * 3 * Vp + v;
        vp[0] += sq[0] * ce; vp[1] += sq[Vp] * ce; vp[2] += sq[2 * Vp] * ce;
    }
    float T[12];
    for (int e = 0; e < 12; ++e) T[e] = 0.0f;
    for (int j = 0; j < K; ++j) {
        const float w = lm.weights[(size_t)j * Vp + v];
        if (w != 0.0f) for (int e = 0; e < 12; ++e) T[e] += w * A[j * 12 + e];
    }
    const float* tr = trans + (size_t)f * 3;
    float* o = out + ((size_t)f * md.V + v) * 3;
    for (int i = 0; i < 3; ++i) o[i] = T[i * 4 + 0] * vp[0] + T[i * 4 + 1] * vp[1] + T[i * 4 + 2] * vp[2] + T[i * 4 + 3] + tr[i];
}

// ---- per-frame preparation: joint transforms + f16 pose features ---------------------------------------
// One wavefront per frame, lane = joint, four frames per workgroup.  Round 6 form -- everything of a frame lives in the wave's
// registers: the lane's rotation vector straight from the pose row (body joints) or as hands_mean + sum_i pose_hand[i] comps[i][.]
// with the f32 component rows fetched in ONE batch of independent loads (the model keeps an f32 copy: rounds 3-5 converted the
// 2 160 f64 components in every workgroup and ran the product as a per-lane LDS loop -- 62 % of the kernel's 15 us went by before
// Rodrigues started); Rodrigues; then the kinematic chain level by level with the parent's world transform fetched ACROSS LANES
// (ds_bpermute, 12 values a level) instead of through LDS arrays with a wave barrier per level (~770 cycles a level).  LDS holds
// only the four frames' f16 feature rows, from which 16-byte fragment pieces leave.
// per-joint constants of k_lbs_prep, packed so that a lane fetches everything it needs about its joint in ONE round of loads:
//   jtab[j] = 16 dwords: {parent (-1: root), rows n <= 16 of the hand-component window, i0, i1 | J_j | J_j - J_parent (root: J_0) | hands_mean of the
//             joint's three coordinates, is-hand-joint};   hcj[j][u] = {comps[i0 + u][3 columns of joint j], 0}, u < 16, zero beyond the window
__global__ void k_pack_jtab(ModelDev md, const float* __restrict__ Jf, const float* __restrict__ hcompf, const float* __restrict__ hmeanf,
                            float* __restrict__ jtab, float* __restrict__ hcj) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= md.K) return;
    int* ji = reinterpret_cast<int*>(jtab + j * 16);
    float* jf = jtab + j * 16;
    const int p = j > 0 ? md.parents[j] : -1;
    const int c0 = 3 * j, bd = md.body_dof, hd = md.hand_dof, nhf = md.nhand_full;
    int i0 = 0, i1 = 0, hand = 0;
    float hm[3] = {0.0f, 0.0f, 0.0f};
    if (c0 >= bd && hd > 0) {
        const int h = c0 - bd;
        hand = 1;
        i0 = min(min(md.col_lo[h], md.col_lo[h + 1]), md.col_lo[h + 2]);
        i1 = max(max(md.col_hi[h], md.col_hi[h + 1]), md.col_hi[h + 2]);
        if (i1 < i0) i1 = i0;
        for (int c = 0; c < 3; ++c) hm[c] = hmeanf[h + c];
        for (int u = 0; u < 16; ++u)
            for (int c = 0; c < 4; ++c) hcj[(j * 16 + u) * 4 + c] = (c < 3 && i0 + u < i1) ? hcompf[(size_t)(i0 + u) * nhf + h + c] : 0.0f;
    } else {
        for (int u = 0; u < 64; ++u) hcj[j * 64 + u] = 0.0f;
    }
    ji[0] = p; ji[1] = min(i1 - i0, 16); ji[2] = i0; ji[3] = i1;
    for (int i = 0; i < 3; ++i) {
        jf[4 + i] = Jf[j * 3 + i];
        jf[8 + i] = Jf[j * 3 + i] - (p >= 0 ? Jf[p * 3 + i] : 0.0f);
        jf[12 + i] = hm[i];
    }
    jf[7] = 0.0f; jf[11] = 0.0f; ji[15] = hand;
}

// sine in the export's preparation: the hardware instruction on the device (v_sin_f32 on t / 2 pi: absolute error ~1e-6 over the rotation
// angles a pose holds, below the f16 quantisation of the features it feeds; the library routine's exact range reduction costs ~50
// instructions a call in a kernel that 4 000 waves run at once), the library's in the host build of the emulation
#if defined(__HIP_DEVICE_COMPILE__)
#define LBS_SIN(x) __sinf(x)
#define LX_KEEP_F(x) __asm__ __volatile__("" : : "v"(x))
#define LX_KEEP_U(x) __asm__ __volatile__("" : : "v"(x))
#else
#define LBS_SIN(x) sinf(x)
#define LX_KEEP_F(x)
#define LX_KEEP_U(x)
#endif
#ifndef LBS_PREP_WAVES
#define LBS_PREP_WAVES 16      // frames (= waves) per workgroup of k_lbs_prep: a whole 16-frame block
#endif
// SH: the frame carries E coefficients of the free shape block (shape[F][E]).  They become its first KSX k-steps of features -- coefficient e
// as the f16 pair (hi, lo) of c_e x sxscale in the columns 3e (hi), 3e + 1 (lo), 3e + 2 (hi), matching k_pack_pfrag_shape; KS counts
// ALL k-steps then, the pose features start at column 32 KSX -- and move the joints, J_f = J + JS . c_f in f32, ahead of the chain
// (lane j: E 16-byte loads of JSf, the coefficients fetched across lanes; the parent's joint across lanes too).
#define LBS_PREP_KSMAX 28      // k-steps of a feature row with a block: 16 (pose, K <= 57) + 12 (3 x 125 shape columns)
template <bool SH>
__global__ __launch_bounds__(64 * LBS_PREP_WAVES, LBS_PREP_WAVES == 16 ? 1 : 4) void k_lbs_prep(ModelDev md, const float* __restrict__ jtab, const float* __restrict__ hcj, const float* __restrict__ hcompf,
                                                   int F, int KS, int KJ,
                                                   const float* __restrict__ pose, const float* __restrict__ trans,
                                                   float* __restrict__ Atr, _Float16* __restrict__ featF, int* __restrict__ varflag, int epoch,
                                                   long long* __restrict__ stamps,
                                                   const float* __restrict__ JSf, const float* __restrict__ shape, int E, int KSX, float sxscale) {
#define PREP_STAMP(K) { if (stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0) stamps[K] = clock64(); }
    constexpr int NFE = (SH ? LBS_PREP_KSMAX : 16) * 32;
    __shared__ __attribute__((aligned(16))) _Float16 s_feat[LBS_PREP_WAVES][NFE];   // the workgroup's frames' feature rows (KS <= 16 k-steps of 32; with a block <= 28), zero padded
    const int fpose = SH ? KSX * 32 : 0;         // column of the first pose feature
    const int K = md.K, wv = threadIdx.x >> 6, tid = threadIdx.x & 63;
    // Workgroup -> frames: a workgroup is 16 waves = one whole 16-frame block of the outputs (768-byte runs of a joint's transforms, 1 KB
    // feature records), completed by one CU in one L2 and leaving it as whole lines.  (What bounds the kernel is the instruction count:
    // 4 000 waves are four a SIMD, and a SIMD issues one vector instruction per ~4.5 cycles whichever wave it comes from -- an empty
    // kernel of this shape takes 2.2 us, one with 2 000 dependent FMAs a wave 16.4 us, tools/ubench_dispatch.hip; this one, ~700 vector +
    // ~300 other instructions a wave, 18-19 us.  Four or sixteen waves a workgroup: the same.)
#if LBS_PREP_WAVES == 16
    const int fbase = (int)blockIdx.x * 16;
#else
    const int fbase = (((int)blockIdx.x >> 5) * 8 + ((int)blockIdx.x & 7)) * 16 + (((int)blockIdx.x >> 3) & 3) * 4;
#endif
    const int fw = fbase + wv;                   // this wave's frame; spare waves behind the last frame redo frame F - 1 and write nothing
    const int f = __builtin_amdgcn_readfirstlane(min(fw, F - 1));
    PREP_STAMP(0)
    for (int q = tid; q < NFE; q += 64) s_feat[wv][q] = (_Float16)0.0f;
    // (no instruction on the device, where a wave's lanes move together; the CPU emulation runs them one after another and meets here:
    //  the features written below must not be zeroed by a lane that comes later)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float* ps = pose + (size_t)f * md.NP;
    const int bd = md.body_dof, nhf = md.nhand_full, hd = md.hand_dof;
    const int j = min(tid, K - 1);               // (lanes beyond the joints shadow joint K - 1 and write nothing)
    const bool act = tid < K;
    // ---- ONE round of independent loads: the joint's record, its window of the hand components, the lane's pose variables of this
    //      frame and of frame 0 (a dependent round trip costs 1-2 000 cycles with 4 000 waves starting at once; round 5 made thirty,
    //      this kernel's first form two)
    const f32x4* jt = reinterpret_cast<const f32x4*>(jtab) + j * 4;
    const f32x4 q0 = jt[0], q1 = jt[1], q2 = jt[2], q3 = jt[3];
    const unsigned* psb = reinterpret_cast<const unsigned*>(ps);
    const unsigned* p0b = reinterpret_cast<const unsigned*>(pose);
    const int c0 = 3 * j, cb = min(c0, max(bd - 3, 0));
    unsigned bv[3], b0[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { bv[i] = psb[cb + i]; b0[i] = p0b[cb + i]; }
    const int hl = bd + min(tid, max(hd - 1, 0));
    const unsigned phb = hd > 0 ? psb[hl] : 0u, ph0 = hd > 0 ? p0b[hl] : 0u;
    float cr0 = 0.0f, cr1 = 0.0f;                // (SH) lane i: coefficients i and 64 + i of this frame (E <= 128)
    if (SH) {
        const float* cf = shape + (size_t)f * E;
        cr0 = cf[min(tid, E - 1)]; cr1 = cf[min(tid + 64, E - 1)];
    }
    // (the elements are copied to scalars first: __builtin_bit_cast applied to a vector ELEMENT expression read element 0 in the host build)
    const float q0x = q0.x, q0z = q0.z, q0w = q0.w, q3w = q3.w;
    const bool hand = __builtin_bit_cast(int, q3w) != 0;
    f32x4 cv[16];
    if (hand) {
#pragma unroll
        for (int u = 0; u < 16; ++u) cv[u] = reinterpret_cast<const f32x4*>(hcj)[j * 16 + u];
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) cv[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int p = __builtin_bit_cast(int, q0x), i0 = __builtin_bit_cast(int, q0z), i1 = __builtin_bit_cast(int, q0w);
    float Jme[3] = {q1.x, q1.y, q1.z}, Jd[3] = {q2.x, q2.y, q2.z};
    if (SH) {   // this frame's joints: J_j + sum_e c_e JS[j][e]; the offset to the parent from the parent's lane
        const f32x4* js = reinterpret_cast<const f32x4*>(JSf) + (size_t)j * E;
        for (int e = 0; e < E; ++e) {
            const float ce = __shfl(e < 64 ? cr0 : cr1, e & 63);
            const f32x4 d = js[e];
            Jme[0] = fmaf(ce, d.x, Jme[0]); Jme[1] = fmaf(ce, d.y, Jme[1]); Jme[2] = fmaf(ce, d.z, Jme[2]);
        }
        const int psrc = max(p, 0);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float jp = __shfl(Jme[i], psrc);
            Jd[i] = p >= 0 ? Jme[i] - jp : Jme[i];
        }
        // the coefficients as features: c x sxscale = hi + lo in f16 (clamped far inside the f16 range)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = tid + 64 * h;
            if (e < E) {
                const float c = fminf(fmaxf((h == 0 ? cr0 : cr1) * sxscale, -32768.0f), 32768.0f);
                const _Float16 chi = (_Float16)c;
                const _Float16 clo = (_Float16)(c - (float)chi);
                s_feat[wv][3 * e] = chi; s_feat[wv][3 * e + 1] = clo; s_feat[wv][3 * e + 2] = chi;
            }
        }
    }
    // ---- which joints MOVE in this call: varflag[j] = epoch as soon as one frame's inputs of joint j differ (bitwise) from frame 0's.
    // A joint nobody marks has the same rotation -- the same nine pose features -- in every frame: its correctives are a constant of the
    // call (k_lbs_still; a body-only solve leaves the 30 hand joints of SMPL-H at the hand prior's mean: chmosh.py:626-647 with
    // optimize_fingers off, the reference's default).  The hand joints share one answer: their rotation vectors depend on the
    // hand-pose variables only.
    if (stamps != nullptr) {   // (development: which of the first loads the wave waits for)
        LX_KEEP_F(q0.x); PREP_STAMP(6)
        LX_KEEP_U(bv[0]); LX_KEEP_U(phb); PREP_STAMP(7)
        LX_KEEP_U(b0[0]); LX_KEEP_U(ph0); PREP_STAMP(8)
        LX_KEEP_F(cv[15].x); PREP_STAMP(9)
    }
    bool hands_differ = __ballot(tid < hd && phb != ph0) != 0ull;
    for (int base = 64; base < hd; base += 64) {   // (hand spaces of more than 64 variables: the same, 64 at a time)
        const int i = min(base + tid, hd - 1);
        hands_differ = hands_differ || __ballot(psb[bd + i] != p0b[bd + i]) != 0ull;
    }
    // ---- the lane's rotation vector: the pose variables themselves (body joints), or hands_mean + pose_hand . components over the
    //      joint's window of component rows, the pose variables fetched across lanes (lane i holds hand variable i)
    float rv[3];
    const float phf = __builtin_bit_cast(float, phb);
    {
        float hv[3] = {q3.x, q3.y, q3.z};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float pu = __shfl(phf, min(i0 + u, 63));       // (every lane takes part; rows past the window have zero components)
#pragma unroll
            for (int c = 0; c < 3; ++c) hv[c] = fmaf(pu, cv[u][c], hv[c]);
        }
        if (hand) {
            for (int i = max(i0 + 16, 0); i < i1; ++i) {          // (windows of more than 16 rows, hand spaces beyond 64 variables: the rest, plainly)
                const float pu = ps[bd + i];
#pragma unroll
                for (int c = 0; c < 3; ++c) hv[c] = fmaf(pu, hcompf[(size_t)i * nhf + (c0 - bd) + c], hv[c]);
            }
            if (hd > 64) {      // (the shuffle above reached variables 0 .. 63 only: redo the first 16 rows from memory)
#pragma unroll
                for (int c = 0; c < 3; ++c) hv[c] = (c == 0 ? q3.x : c == 1 ? q3.y : q3.z);
                for (int i = i0; i < i1; ++i) {
                    const float pu = ps[bd + i];
#pragma unroll
                    for (int c = 0; c < 3; ++c) hv[c] = fmaf(pu, hcompf[(size_t)i * nhf + (c0 - bd) + c], hv[c]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) rv[i] = hand ? hv[i] : __builtin_bit_cast(float, bv[i]);
    }
    if (act && (hand ? hands_differ : (bv[0] != b0[0] || bv[1] != b0[1] || bv[2] != b0[2]))) varflag[j] = epoch;
    PREP_STAMP(1)
    // ---- Rodrigues: the local rotation Rl, and R - I (without the cancellation) as f16 features
    float Rl[9];
    {
        const float x = rv[0], y = rv[1], z = rv[2];
        const float t2 = x * x + y * y + z * z;
        float a, b;
        if (t2 < 1e-6f) { a = 1.0f - t2 / 6.0f; b = 0.5f - t2 / 24.0f; }
        else { const float t = sqrtf(t2); a = LBS_SIN(t) / t; const float sh = LBS_SIN(0.5f * t); b = 2.0f * sh * sh / t2; }   // (1 - cos t = 2 sin^2 (t / 2): no cancellation at small angles)
        const float K2[9] = {x * x - t2, x * y, x * z, x * y, y * y - t2, y * z, x * z, y * z, z * z - t2};
        const float Km[9] = {0.0f, -z, y, z, 0.0f, -x, -y, x, 0.0f};
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const float id = (e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f;
            const float d = a * Km[e] + b * K2[e];
            Rl[e] = id + d;
            if (act && j >= 1) s_feat[wv][fpose + (j - 1) * 9 + e] = (_Float16)d;
        }
    }
    PREP_STAMP(2)
    // ---- kinematic chain by pointer jumping: every lane holds the transform (R, t) from its joint's frame to the frame of an ANCHOR
    // ancestor -- at first its parent: (Rl_j, J_j - J_parent); the root: (Rl_0, J_0), no anchor -- and in every round composes it with the
    // anchor's own (fetched across lanes: 12 values + the anchor's anchor) and adopts the anchor's anchor: the distance doubles, so
    // ceil(log2(depth + 1)) rounds (4 for the 10 levels of SMPL-H) replace one round per tree level
    float Rw[9], tw[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rw[e] = Rl[e];
#pragma unroll
    for (int i = 0; i < 3; ++i) tw[i] = Jd[i];
    int anchor = act ? p : -1;
    for (int reach = 1; reach <= md.maxdepth; reach *= 2) {
        const int src = max(anchor, 0);
        float pr[9], pt[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) pr[e] = __shfl(Rw[e], src);
#pragma unroll
        for (int i = 0; i < 3; ++i) pt[i] = __shfl(tw[i], src);
        const int pa = __shfl(anchor, src);
        if (anchor >= 0) {
            float Rn[9], tn[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Rn[i * 3 + c] = pr[i * 3 + 0] * Rw[c] + pr[i * 3 + 1] * Rw[3 + c] + pr[i * 3 + 2] * Rw[6 + c];
                tn[i] = pr[i * 3 + 0] * tw[0] + pr[i * 3 + 1] * tw[1] + pr[i * 3 + 2] * tw[2] + pt[i];
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) Rw[e] = Rn[e];
#pragma unroll
            for (int i = 0; i < 3; ++i) tw[i] = tn[i];
            anchor = pa;
        }
    }
    PREP_STAMP(3)
    if (act && fw < F) {   // A_j = [Rw | tw - Rw J_j + trans]  (sum_j w_j = 1 lets the root translation ride in every joint), row major:
                           // three 16-byte pieces (R_i0, R_i1, R_i2, t_i) -- each float is one B operand of the export kernel's blend
        f32x4* o = reinterpret_cast<f32x4*>(Atr + (((size_t)(f >> 4) * KJ + j) * 16 + (f & 15)) * 12);
        const float* tr = trans + (size_t)f * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float r0 = Rw[i * 3 + 0], r1 = Rw[i * 3 + 1], r2 = Rw[i * 3 + 2];
            o[i] = f32x4{r0, r1, r2, tw[i] - (r0 * Jme[0] + r1 * Jme[1] + r2 * Jme[2]) + tr[i]};
        }
    }
    PREP_STAMP(4)
    // B fragments of v_mfma_f32_16x16x32_f16: features 8 g .. 8 g + 7 of frame f are the 16 bytes of record (f / 128, g / 4,
    // (f / 16) % 8), lane (f % 16) + 16 (g % 4).  The workgroup's frames are consecutive lanes: thread (g, frame) writes
    // one 16-byte piece, the frames' threads one contiguous run (the first version wrote every feature as a 2-byte store of its own: 2.4 M write
    // requests per call, the waves a third of their time at the issue stage behind them).
    __syncthreads();
    {
        const int fi = threadIdx.x & (LBS_PREP_WAVES - 1), fo = fbase + fi;
        int g = threadIdx.x / LBS_PREP_WAVES;
        do {   // (one piece a thread without a block: KS <= 16; with one, up to 28 k-steps = 112 pieces a frame)
            if (g < KS * 4 && fo < F) {
                const f32x4 piece = *reinterpret_cast<const f32x4*>(&s_feat[fi][g * 8]);
                _Float16* dst = featF + ((((size_t)(fo >> 7) * KS + (g >> 2)) * 8 + ((fo >> 4) & 7)) * 64 + (fo & 15) + 16 * (g & 3)) * 8;
                *reinterpret_cast<f32x4*>(dst) = piece;
            }
            g += 64;
        } while (SH && g < KS * 4);
    }
    PREP_STAMP(5)
#undef PREP_STAMP
}

// ---- the export kernel ------------------------------------------------------------------------------------
// k_lbs_export: a workgroup = 4 waves (one per SIMD, <= 256 registers, 80 KB of LDS) so that TWO workgroups share a CU, each with
// its own tile of 64 vertices x 128 frames, and run in antiphase: while one is in its k-loop (matrix pipe: 360 MFMAs per wave) the
// other is in its blend epilogue (vector pipe + LDS).  The two pipes issue side by side from different waves of a SIMD, so a CU's
// tile pair costs max(matrix, vector) instead of their sum -- the round-3/4 kernel (ONE workgroup per CU, all eight waves in the
// same phase) paid the sum: 18 k cycles of k-loop with the vector pipe idle, then 26 k of epilogue with the matrix pipe idle.
//
// Wave w of a tile owns the vertex GROUP w: 16 of the tile's 64 vertices, chosen at model-prepare time (group_tiles below) so that
// a group depends on as few joints as possible -- its JOINT LIST, padded to rounds of LX_JR = 4 joints.  The MFMA accumulators are
// lane = frame, register = vertex (as before), and the blend runs over the group's joint list instead of over each vertex's own
// influences: per 16-frame block and round the wave copies the four joints' transforms (4 x 768 B, gathered by LDS-DMA with
// per-lane source addresses) into a wave-private LDS buffer, every lane reads its frame's 4 x 48 B ONCE for all four of its
// vertices (the round-3 form read 4 vertices x 4 influences x 48 B: the LDS pipe and ~450 instructions per block) and accumulates
// T_v += w_vj A_j as packed FMAs (v_pk_fma_f32: the transforms are stored as the pairs (R00,R10) (R01,R11) (R02,R12) (t0,t1)
// (R20,R21) (R22,t2), the weight is broadcast by op_sel) -- 96 packed FMAs per round, 24 instructions to apply T to the four
// corrected rest positions.  Vertices whose joints are not in a round have weight 0 there.  Nothing in the epilogue is shared
// between waves except the result exchange (un-permutes the group order, whole 768-byte tile rows leave as 16-byte streaming
// stores): ONE workgroup barrier per 16-frame block; the transforms need none (a wave waits for its own DMA with a counted vmcnt).
#define LX_TV 64             // vertices per tile (16 per wave)
#define LX_TF 128            // frames per tile (8 MFMA column tiles of 16)
#ifndef LX_XP
#define LX_XP 194            // dwords per row of the result exchange: 64 vertices x 3 + 2: the 16 frame rows of a two-dword write start
                             // on 16 distinct even banks
#endif
#define LX_JR 4              // joints per blend round
#ifndef LX_STAUX
#define LX_STAUX 2           // cache policy of the row stores: 2 = nt (streaming)
#endif
#ifndef LX_NRMAX
#define LX_NRMAX 6           // rounds per group the kernel's LDS tables hold (24 joints per 16 vertices; else the plain kernel runs)
#endif
#define LX_RING 3            // slots of the feature ring
#define LX_CHUNK 8192        // bytes of one k-step's feature fragments: 8 frame blocks x 64 lanes x 16 B
#define LX_JBYTES 768        // one joint's transforms for 16 frames (16 x 12 floats)
#define LX_OFF_SX (LX_RING * LX_CHUNK)                         // result exchange, two buffers of 16 rows
#define LX_SXBYTES (16 * LX_XP * 4)
#define LX_OFF_W (LX_OFF_SX + 2 * LX_SXBYTES)                  // weights [group][round][slot 16][joint 4] f32 (rounds >= 1 read them here)
#define LX_OFF_J (LX_OFF_W + 4 * LX_NRMAX * 256)               // joint lists [group][round][4] (byte offsets j x 768)
#define LX_LDS_BYTES (LX_OFF_J + 4 * LX_NRMAX * LX_JR * 4)     // 55 936 B: two workgroups per CU

#define LBS_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// (wave_barrier: no instruction on the device, where a wave's lanes move together; the CPU emulation runs lanes one after another and
//  meets there -- a lane reads LDS bytes that the other lanes of its wave wrote)
#define LBS_WAVE_SYNC() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// LX_OPAQUE(x): the compiler may not treat x as loop-invariant behind this point (it would hoist every lane-only address computation
// of the epilogue out of the tile loop and park the results in registers the loops need -- measured: 35 spills ahead of the tile
// loop, reloaded inside the block loop); on the host / in the emulation nothing
#if defined(__HIP_DEVICE_COMPILE__)
#define LX_OPAQUE(x) __asm__ __volatile__("" : "+v"(x))
#define LX_KEEP(x) __asm__ __volatile__("" : : "v"(x))   // x stays in its registers, unused by anything else, up to here
#else
#define LX_OPAQUE(x)
#define LX_KEEP(x)
#endif

// ---- per call: the correctives of the joints that do not move ---------------------------------------------------------------------
// k_lbs_prep has marked the joints whose rotation differs between frames (varflag[j] == epoch).  The pose features of the others are
// the same in every frame, so their correctives  sum_{k >= 32 kseff} posedirs[v][k] feature[k]  are one constant per vertex for the
// whole call: one wavefront per vertex group evaluates them once -- the k-steps behind the last moving joint, on the fragments the
// export kernel would read, against frame 0's features -- and writes  pscale x (rest + still correctives)  in the layout of the rest
// positions (tab_vsc): the start value of the export kernel's accumulators, whose k-loop then ends at kseff.  A body-only Stage-II
// result (the reference's default: optimize_fingers off) keeps the 30 hand joints of SMPL-H still: 9 of 15 k-steps.
// (SH: the extended layout -- KSX shape k-steps, which change per frame and so always stay in the export's loop, in front of the pose k-steps)
template <bool SH>
__global__ __launch_bounds__(64, 1) void k_lbs_still(Lbs32Model lm, const int* __restrict__ varflag, int epoch, int all_move) {
    const int lane = threadIdx.x, g = blockIdx.x, ksx = SH ? lm.KSX : 0, KS = lm.KS + ksx, q4 = lane >> 4, fl = lane & 15;
    int kseff = KS;
    if (!all_move) {
        const bool moves = lane >= 1 && lane < lm.K && varflag[min(lane, lm.K - 1)] == epoch;
        const unsigned long long mv = __ballot(moves);
        const int jl = mv ? 63 - __builtin_clzll(mv) : 0;
        kseff = min(KS, ksx + (9 * jl + 31) / 32);
    }
    const __amdgpu_buffer_rsrc_t rs_feat = __builtin_amdgcn_make_buffer_rsrc((void*)lm.featF, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_pf = __builtin_amdgcn_make_buffer_rsrc((void*)(SH ? lm.PfragX : lm.Pfrag), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_tab = __builtin_amdgcn_make_buffer_rsrc((void*)lm.tables, 0, 0x7fffffff, 0x00020000);
    f32x4 vs[4], acc[3];
#pragma unroll
    for (int r = 0; r < 4; ++r) vs[r] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_tab, (unsigned)(4 * q4 + r) * 16u, lm.tab_vshs + (unsigned)g * 256u, 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = f32x4{vs[0][c], vs[1][c], vs[2][c], vs[3][c]};
    const unsigned ap = (unsigned)(g * 3 * KS) * 1024u;
    for (int kc = kseff; kc < KS; kc += 10) {    // (straight-line batches of ten steps -- one round trip for the nine still steps of a body-only
                                                 //  SMPL-H export; past the last step the last one again with a zero B operand)
        half8 ca[10][3], cb[10];
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const unsigned kk = (unsigned)min(kc + u, KS - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) ca[u][c] = (half8)__builtin_amdgcn_raw_buffer_load_b128(rs_pf, lane * 16u, ap + (c * (unsigned)KS + kk) * 1024u, 0);
            const u32x4 braw = __builtin_amdgcn_raw_buffer_load_b128(rs_feat, lane * 16u, kk * LX_CHUNK, 0);   // frame tile 0, frame block 0
            const unsigned keep = (kc + u < KS) ? 0xffffffffu : 0u;
            cb[u] = (half8)(braw & u32x4{keep, keep, keep, keep});
        }
#pragma unroll
        for (int u = 0; u < 10; ++u)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ca[u][c], cb[u], acc[c], 0, 0, 0);
    }
    if (fl == 0) {   // column 0 = frame 0; register r = vertex slot 4 q4 + r
        float* o = reinterpret_cast<float*>(lm.tables + lm.tab_vsc) + ((size_t)g * 16 + 4 * q4) * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(o + r * 4) = f32x4{acc[0][r], acc[1][r], acc[2][r], 0.0f};
    }
}

// SH (an instantiation of its own; the one without is the code as it was): the call carries coefficients of the free shape block.  The
// k-loop is the same loop over a longer row: KSX shape k-steps in front (PfragX / k_lbs_prep<true>'s features), always run, then the
// moving joints' pose k-steps.
template <bool SH>
__global__ __launch_bounds__(256, 2) void k_lbs_export(Lbs32Model lm, int V, int F, int NVT, int NFT, float* __restrict__ out, const int* __restrict__ varflag, int epoch,
                                                     long long* __restrict__ dbgbuf, int dbg) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ksx = SH ? lm.KSX : 0;
    const int KS = SH ? lm.KS + ksx : lm.KS, NRM = lm.NRM;
    // k-steps [kseff, KS) hold features of joints that do not move in this call (k_lbs_prep's varflag): the same in every frame -- their
    // correctives are a per-vertex constant of the call, which k_lbs_still has added to the rest positions the accumulators start at
    // (tab_vsc); the k-loop runs the first kseff steps.  (dbg & 8: treat every joint as moving.)
    int kseff = KS;
    if (!(dbg & 8)) {
        const bool moves = lane >= 1 && lane < lm.K && varflag[min(lane, lm.K - 1)] == epoch;
        const unsigned long long mv = __ballot(moves);
        const int jl = mv ? 63 - __builtin_clzll(mv) : 0;          // the last moving joint: its features end at 9 jl
        kseff = __builtin_amdgcn_readfirstlane(min(KS, SH ? ksx + (9 * jl + 31) / 32 : (9 * jl + 31) / 32));
    }
    const unsigned tlb = (unsigned)lm.KJ * LX_JBYTES;      // bytes of one 16-frame block's transforms
    char* ring = lds_raw;                                  // [LX_RING][8 frame blocks][64 lanes][16 B]
    char* Sx = lds_raw + LX_OFF_SX;                        // [2][16 frames][LX_XP] f32
    // XCD-aware tile order.  Workgroup b runs on XCD b % 8; XCD x owns the vertex tiles {x, x + 8, ...}, whose posedirs fragments
    // stay in that XCD's L2, and its workgroups walk (frame tile, vertex tile) side by side.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;
    // Whole vertex tiles per XCD (SMPL-H: 108 = 13 x 8 + 4, so four XCDs carry 14 x NFT tiles against 13 x NFT and end ~20 us behind).
    // (dbg & 4: the even deal -- the partial round of vertex tiles dealt out as (vertex tile, frame tile) pairs, an eighth to every XCD
    //  in one contiguous run.  Measured twice, rounds 5 and 6, with two different kernels: every XCD then ends together -- and LATER
    //  (199.7 against 190.5 us per call): the XCDs that finish early leave the others a faster memory side for their last tiles.)
    const int nvb = NVT >> 3, nvr = NVT & 7;
    const bool olddeal = (dbg & 4) == 0;
    const int NVX = olddeal ? (NVT - xcd + 7) >> 3 : nvb;
    const int nreg = NVX * NFT;
    const int upairs = olddeal ? 0 : nvr * NFT, ulo = xcd * upairs / 8, uhi = (xcd + 1) * upairs / 8;
    const int ntiles = nreg + (uhi - ulo);
    const float isc = lm.inv_pscale;
    const int q4 = lane >> 4, fl = lane & 15;
    // (MOSHII_LBS_STOP=16: workgroup 0 leaves clock stamps of its phases in dbgbuf -- tools/lbs_bench.py prints them; the output stays complete)
#define LX_STAMP(K) { if (stamping && tid == 0) dbgbuf[stamp_tile * 24 + (K)] = clock64(); }
    const bool stamp_wg = (dbg & 16) && blockIdx.x == 0;
    bool stamping = false;
    int stamp_tile = 0;
    const long long wg_t0 = (dbg & 32) ? wall_clock64() : 0;   // (MOSHII_LBS_STOP=32: every workgroup leaves its start / end time in dbgbuf)
    // No LDS-DMA anywhere in this kernel (rounds 3/4 fetched the transforms with global_load_lds; the first form of this kernel the
    // features as well).  Measured this round: (1) the compiler books a FLAT-encoded LDS load as an access to both memories and turns
    // every wait it inserts while one is in flight into a full drain of both counters -- no read-ahead survives; (2) as BUFFER loads
    // (buffer_load_dwordx4 ... lds) its waits stay counted, but counted waits of my own across LDS loads + register loads + stores
    // returned stale LDS on the device (vmcnt(2) wrong, vmcnt(0) right: the three kinds do not retire in issue order relative to each
    // other); (3) MI355X_MICROARCH.md puts the landing rate of LDS-DMA at ~12 B/clk per CU, a fifth of what plain loads deliver --
    // this kernel wants 20-25.  So everything comes through registers: plain loads whose waits the compiler counts, then ds_write.
    // All hot loads and stores are BUFFER instructions: wave-uniform resource (4 SGPRs) + scalar offset + ONE 32-bit lane offset.  As
    // global_load / global_store the compiler kept a 64-bit address per lane and per stream in registers across the loops (hoisted out
    // of the tile loop as loop invariants: ~30 registers, spilled and reloaded inside the k-steps).
    // Resource words: base, no stride, 2^31 - 1 bytes, raw 32-bit data format.
    const __amdgpu_buffer_rsrc_t rs_atr = __builtin_amdgcn_make_buffer_rsrc((void*)lm.Atr, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_feat = __builtin_amdgcn_make_buffer_rsrc((void*)lm.featF, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_pf = __builtin_amdgcn_make_buffer_rsrc((void*)(SH ? lm.PfragX : lm.Pfrag), 0, 0x7fffffff, 0x00020000);
    // (the small per-tile tables as well -- ONE kind of vector load in the kernel -- and all of them behind one resource: the model keeps
    //  them in one allocation, lm.tab_* are the tables' byte offsets in it; a resource is four scalar registers)
    const __amdgpu_buffer_rsrc_t rs_tab = __builtin_amdgcn_make_buffer_rsrc((void*)lm.tables, 0, 0x7fffffff, 0x00020000);
    // The blend T_v = sum_j w_vj A_j runs on v_mfma_f32_16x16x4_f32 (round 6): per 16-frame block and ROUND of four list joints,
    // D[vertex slot 4 q4 + r][frame fl] += W[slot][joint k] . A_k[frame][entry] for each of the 12 entries of the 3 x 4 transforms --
    // twelve matrix instructions where rounds 3-5 issued 96 packed (or 192 plain) vector FMAs per lane set.  The B operand of entry e
    // is ONE float per lane: lane (fl, k = lane >> 4) holds entry e of list joint k for frame fl -- the lane's own 48 bytes of that
    // joint's 16 x 48-byte run in Atr, three 16-byte loads straight from L2 into operand registers (no LDS staging, no wave sync);
    // the A operand is the lane's weight W[slot fl][joint k] (x 1 / pscale for the rotation entries: the accumulators carry
    // pscale x (rest + corrective)).  Accumulator layout = the k-loop's: lane = frame, register r = vertex slot 4 q4 + r.
    f32x4 sg[3];   // the NEXT item's transforms (this lane's joint, this lane's frame), loaded one item ahead
    auto load_item = [&](unsigned block, unsigned off) {   // block: byte offset of the 16-frame block in Atr (wave-uniform); off: lane offset
#pragma unroll
        for (int p = 0; p < 3; ++p) sg[p] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_atr, off + 16u * p, block, 0);
    };
    const int* ljt = reinterpret_cast<const int*>(lds_raw + LX_OFF_J) + wv * NRM * LX_JR;   // this group's joint list in LDS
    half8 aS[3][3], bS[8];
    f32x4 gS[2][2];
#define LX_LD_A(SET, KSTEP) { const unsigned kk_ = (unsigned)min((KSTEP), kseff - 1); _Pragma("unroll") for (int c = 0; c < 3; ++c) \
        aS[SET][c] = (half8)__builtin_amdgcn_raw_buffer_load_b128(rs_pf, lane * 16u, ap + (c * (unsigned)KS + kk_) * 1024u, 0); __builtin_amdgcn_sched_barrier(0); }
#define LX_LD_G(SET, KSTEP) { const unsigned kk_ = (unsigned)min((KSTEP), kseff - 1); gS[SET][0] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_feat, tid * 16u, fp + kk_ * LX_CHUNK, 0); \
        gS[SET][1] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_feat, tid * 16u, fp + kk_ * LX_CHUNK + 4096u, 0); }
#define LX_ST_G(SET, SLOT) { *reinterpret_cast<f32x4*>(ring + (SLOT) * LX_CHUNK + tid * 16) = gS[SET][0]; *reinterpret_cast<f32x4*>(ring + (SLOT) * LX_CHUNK + (tid + 256) * 16) = gS[SET][1]; }
    // (four B-fragment registers: the fragments of frame blocks 0 .. 3 are read behind the barrier, block T + 4 goes into block T's
    //  register as soon as its three MFMAs are issued -- 144 cycles of MFMAs ahead of its own)
#ifdef LX_DBG_B8
#define LX_BI(T) (T)
#else
#define LX_BI(T) ((T) & 3)
#endif
#define LX_LD_B1(SLOT, T) { bS[LX_BI(T)] = *reinterpret_cast<const half8*>(ring + (SLOT) * LX_CHUNK + (T) * 1024 + lane * 16); }
#define LX_LD_B(SLOT) { LX_LD_B1(SLOT, 0) LX_LD_B1(SLOT, 1) LX_LD_B1(SLOT, 2) LX_LD_B1(SLOT, 3) }
#define LX_MMA_T(ASET, T) { _Pragma("unroll") for (int c = 0; c < 3; ++c) acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aS[ASET][c], bS[LX_BI(T)], acc[T][c], 0, 0, 0); __builtin_amdgcn_sched_barrier(0); }
    // Step t.  Chunk c lives in ring slot c % 3.  Barrier: chunk t (and t + 1) are visible, every wave has left chunk t - 1; read the eight
    // B fragments of chunk t, drop chunk t + 2 (fetched two steps ago) into the slot chunk t - 1 occupied, fetch chunk t + 4 and the posedirs
    // fragments of step t + 2; the memory instructions sit BETWEEN the step's 24 MFMAs (a load does not leave the issue stage while the
    // address unit is busy with other waves' loads).
#define LX_STEP(S, KSTEP) { \
        LBS_LDS_BARRIER(); \
        LX_LD_B((S) % 3) __builtin_amdgcn_sched_barrier(0); \
        LX_MMA_T((S) % 3, 0) LX_LD_B1((S) % 3, 4) \
        if ((KSTEP) + 2 < kseff) { LX_ST_G((S) % 2, ((S) + 2) % 3) } __builtin_amdgcn_sched_barrier(0); \
        LX_MMA_T((S) % 3, 1) LX_LD_B1((S) % 3, 5) \
        if ((KSTEP) + 4 < kseff) { LX_LD_G((S) % 2, (KSTEP) + 4) } __builtin_amdgcn_sched_barrier(0); \
        LX_MMA_T((S) % 3, 2) LX_LD_B1((S) % 3, 6) \
        if ((KSTEP) + 2 < kseff) LX_LD_A(((S) + 2) % 3, (KSTEP) + 2) \
        LX_MMA_T((S) % 3, 3) LX_LD_B1((S) % 3, 7) __builtin_amdgcn_sched_barrier(0); \
        LX_MMA_T((S) % 3, 4) LX_MMA_T((S) % 3, 5) LX_MMA_T((S) % 3, 6) LX_MMA_T((S) % 3, 7) }
    unsigned off0 = 0;   // this lane's offset in a 16-frame block of transforms for the tile's round 0: its list joint + its frame
    for (int idx = slot; idx < ntiles; idx += nslots) {
        int ft, vt;
        if (idx < nreg) { ft = idx / NVX; vt = xcd + 8 * (idx - ft * NVX); }
        else { const int u = ulo + idx - nreg, e = u / NFT; ft = u - e * NFT; vt = 8 * nvb + e; }
        const int f0 = ft * LX_TF, v0 = vt * LX_TV, gi = vt * 4 + wv;
        if (stamp_wg) { stamp_tile = (idx - slot) / nslots; stamping = stamp_tile < 8; }
        LX_STAMP(0)
        if (stamping && tid == 0) dbgbuf[stamp_tile * 24 + 12] = wall_clock64();   // (100 MHz: the shader clock the stamps ran at)
        const int nr = __builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_raw_buffer_load_b32(rs_tab, 0u, lm.tab_gnr + (unsigned)gi * 4u, 0));
        // ---- the tile's tables: the four groups' weights and joint lists into LDS (every wave is past the previous tile's last block)
        for (int i = tid; i < 64 * NRM; i += 256) {   // (4 groups x NRM rounds x 16 slots, 16 bytes each)
            const f32x4 wrow = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_tab, (unsigned)i * 16u, lm.tab_gw + (unsigned)(vt * 64 * NRM) * 16u, 0);
            *reinterpret_cast<f32x4*>(lds_raw + LX_OFF_W + i * 16) = wrow;
        }
        if (tid < 4 * NRM * LX_JR) reinterpret_cast<int*>(lds_raw + LX_OFF_J)[tid] = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_tab, tid * 4u, lm.tab_gjid + (unsigned)(vt * 4 * NRM * LX_JR) * 4u, 0);
        // this lane's four vertices (slots 4 q4 .. 4 q4 + 3 of the group): exchange columns and scaled rest positions -- the accumulators
        // start AT the rest position (x pscale), so the k-loop delivers rest + corrective in one piece
        f32x4 acc[8][3];
        const unsigned ap = (unsigned)(gi * 3 * KS) * 1024u;      // byte offset of the group's fragments in Pfrag
        const unsigned fp = (unsigned)(ft * KS) * LX_CHUNK;      // byte offset of the frame tile's chunks in featF
        {
            f32x4 vs[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) vs[r] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_tab, (unsigned)(4 * q4 + r) * 16u, lm.tab_vsc + (unsigned)gi * 256u, 0);
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[t][c] = f32x4{vs[0][c], vs[1][c], vs[2][c], vs[3][c]};
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- main loop over the moving joints' k-steps: acc[t][c] (16 vertices x 16 frames) += Pfrag(group, c, ks) x featF(t, ks)
        if (kseff > 0) {
            LX_LD_G(0, 0) LX_LD_G(1, 1) LX_LD_A(0, 0) LX_LD_A(1, 1)
            LX_ST_G(0, 0) LX_ST_G(1, 1)
            LX_LD_G(0, 2) LX_LD_G(1, 3)
        }
        LX_STAMP(1)
        int ks = 0;
        for (; ks + 6 <= kseff; ks += 6) {
            LX_STEP(0, ks) LX_STEP(1, ks + 1) LX_STEP(2, ks + 2) LX_STEP(3, ks + 3) LX_STEP(4, ks + 4) LX_STEP(5, ks + 5)
        }
        if (ks < kseff) { LX_STEP(0, ks) ++ks; }
        if (ks < kseff) { LX_STEP(1, ks) ++ks; }
        if (ks < kseff) { LX_STEP(2, ks) ++ks; }
        if (ks < kseff) { LX_STEP(3, ks) ++ks; }
        if (ks < kseff) { LX_STEP(4, ks) ++ks; }
        LX_STAMP(2)
        // what only the epilogue needs is fetched behind the k-loop (held across it these 19 registers were spilled; the first item of a
        // tile waits for them -- the CU's other workgroup runs meanwhile): the lane's exchange columns, its offsets in a round-0 block
        // of transforms, the transforms of the first item
        const u32x4 xo = __builtin_amdgcn_raw_buffer_load_b128(rs_tab, q4 * 16u, lm.tab_gx + (unsigned)gi * 64u, 0);
        {
            unsigned lane_o = lane;
            LX_OPAQUE(lane_o);
            off0 = __builtin_amdgcn_raw_buffer_load_b32(rs_tab, (lane_o >> 4) * 4u, lm.tab_gjid + (unsigned)(gi * NRM * LX_JR) * 4u, 0) + (lane_o & 15u) * 48u;
        }
        // round 0's weights as the A operand: W[slot fl][joint q4], and the same x 1 / pscale for the rotation entries
        const float w0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_tab, (unsigned)(fl * 16 + q4 * 4), lm.tab_gw + (unsigned)(gi * NRM) * 256u, 0));
        const float w0s = w0 * isc;
        load_item((unsigned)ft * 8u * tlb, off0);
        if (dbg & 1) {   // (MOSHII_LBS_STOP=1: stop behind the k-loop)
            float sacc = 0.0f;
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) sacc += acc[t][c][0] + acc[t][c][1] + acc[t][c][2] + acc[t][c][3];
            if (sacc == 123.456f) out[0] = sacc + (float)xo[0] + sg[0].x + sg[1].y + sg[2].z + w0s;
            LBS_LDS_BARRIER();
            continue;
        }
        // ---- epilogue: eight blocks of 16 frames x (this group's rounds).  The block body is expanded eight times (the accumulators are
        // registers: a rolled loop had to copy a block's 12 out through a branch tree -- ~60 moves per block).
        const unsigned abase = (unsigned)ft * 8u * tlb;   // byte offset of the tile's first 16-frame block in Atr
        const int nfl = min(LX_TV, V - v0) * 3;   // valid floats of a tile row
        const bool full = (f0 + LX_TF <= F) && (nfl == LX_TV * 3) && (dbg & 2) == 0;   // interior tile
        // row stores: a block's 16 rows x 768 B are 768 16-byte pieces, three per thread: piece k = 256 s + tid lies in row k / 48
        // (resource = the tile's first row: lane offsets stay below 2^31 whatever the size of the whole output)
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)(out + ((size_t)f0 * V + v0) * 3), 0, 0x7fffffff, 0x00020000);
        const unsigned rowb = (unsigned)V * 12u;   // bytes of an output row
        unsigned rp0, rr0;                         // piece 0 of this thread: row tid / 48, column piece tid % 48
        { unsigned tid_o = tid; LX_OPAQUE(tid_o); rr0 = tid_o / 48u; rp0 = tid_o - rr0 * 48u; }
        f32x4 rv[3];
        auto row_read = [&](int t) {   // the thread's three pieces of block t's rows, out of the exchange
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const unsigned pc = rp0 + 16u * s, w = pc >= 48u ? 1u : 0u, piece = pc - 48u * w, row = rr0 + 5u * s + w;
#if LX_XP % 4 == 0
                rv[s] = *reinterpret_cast<const f32x4*>(Sx + (t & 1) * LX_SXBYTES + row * (LX_XP * 4) + piece * 16);
#else
                const f32x2* sp = reinterpret_cast<const f32x2*>(Sx + (t & 1) * LX_SXBYTES + row * (LX_XP * 4) + piece * 16);
                const f32x2 lo = sp[0], hi = sp[1];
                rv[s] = f32x4{lo.x, lo.y, hi.x, hi.y};
#endif
            }
        };
        // The three stores go out back to back (addresses first); their data registers rv stay untouched until the stores have RETIRED:
        // s_waitcnt vmcnt(0) + LX_KEEP(rv) -- at once (`wait`: a tile's last block), or at the start of the next block, where the wave
        // waits for its transforms anyway.  Measured on the device: with ordinary code behind a buffer_store_dwordx4 -- the compiler
        // re-uses its data registers two wait states later, which is what the ISA asks for -- single floats of the stored pieces
        // arrived wrong in memory (lanes 12 .. 15 of every 16, only in the workgroup that shares its CU's address unit with an older
        // one, a few thousand floats per export): the unit reads a store's data out of the registers later than that when it is backed up.
        // lane offsets of the thread's three pieces in the tile's output rows (block-independent: the block is the scalar offset)
        unsigned voff[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const unsigned pc = rp0 + 16u * s, w = pc >= 48u ? 1u : 0u, piece = pc - 48u * w, row = rr0 + 5u * s + w;
            voff[s] = row * rowb + piece * 16u;
        }
        const int wmode = (dbg & 2) ? 0 : full ? 1 : 2;    // (MOSHII_LBS_STOP=2: no row stores) / interior tile / edge tile
        auto row_write = [&](int t, bool wait) {
            const unsigned soff = (unsigned)(16 * t) * rowb;
            __builtin_amdgcn_sched_barrier(0);
            if (wmode == 1) {
                // interior tile: three unconditional streaming stores (nt: the output must not evict the posedirs fragments the k-loop
                // re-reads from L2).  (Round 5's form decided per store and per debug flag: ~15 scalar branches per block, and a taken
                // branch costs the wave ~30 cycles: the three stores took 480 cycles to issue.)
#pragma unroll
                for (int s = 0; s < 3; ++s) __builtin_amdgcn_raw_buffer_store_b128((u32x4)rv[s], rs_out, voff[s], soff, LX_STAUX);
            } else if (wmode == 2) {
#pragma nounroll
                for (int s = 0; s < 3; ++s) {
                    const unsigned pc = rp0 + 16u * s, w = pc >= 48u ? 1u : 0u, piece = pc - 48u * w, row = rr0 + 5u * s + w;
                    const f32x4 val = s == 0 ? rv[0] : s == 1 ? rv[1] : rv[2];
                    if (f0 + 16 * t + (int)row < F) {
                        if ((int)piece * 4 + 4 <= nfl) __builtin_amdgcn_raw_buffer_store_b128((u32x4)val, rs_out, row * rowb + piece * 16u, soff, 2);
                        else {   // a piece that straddles the end of a partial vertex tile's rows: float by float
                            float* o = out + ((size_t)(f0 + 16 * t + (int)row) * V + v0) * 3 + piece * 4;
                            for (int e = 0; e < 4; ++e) if ((int)piece * 4 + e < nfl) o[e] = val[e];
                        }
                    }
                }
            }
            if (wait) { __builtin_amdgcn_s_waitcnt(0x0F70); LX_KEEP(rv[0]); LX_KEEP(rv[1]); LX_KEEP(rv[2]); }   // vmcnt(0)
            __builtin_amdgcn_sched_barrier(0);
        };
        f32x4 T[3][4];     // T[c][e][r]: entry (c, e) of the blended 3 x 4 transform of vertex slot 4 q4 + r for this lane's frame
        const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
        // Block t: wait for everything in flight (vmcnt(0): explicit, because the compiler would count its own wait for the loads --
        // vmcnt(N), N = the vector-memory instructions issued behind them -- as if everything retired in issue order, and on this
        // device a store issued behind a load can retire ahead of it): this block's round-0 transforms are in sg, the previous block's
        // row stores have read rv.  Twelve matrix instructions; the next item's loads (a whole block to arrive in); the previous
        // block's rows out of the exchange and on their way; further rounds accumulate into T; apply; one workgroup barrier.
#define LX_BLEND(WS, WP, CIN) { \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) { \
            T[c][0] = __builtin_amdgcn_mfma_f32_16x16x4f32((WS), sg[c].x, (CIN) ? zero4 : T[c][0], 0, 0, 0); \
            T[c][1] = __builtin_amdgcn_mfma_f32_16x16x4f32((WS), sg[c].y, (CIN) ? zero4 : T[c][1], 0, 0, 0); \
            T[c][2] = __builtin_amdgcn_mfma_f32_16x16x4f32((WS), sg[c].z, (CIN) ? zero4 : T[c][2], 0, 0, 0); \
            T[c][3] = __builtin_amdgcn_mfma_f32_16x16x4f32((WP), sg[c].w, (CIN) ? zero4 : T[c][3], 0, 0, 0); \
        } }
        // apply: out_v = T_v . (p_v, 1), p_v = pscale x (rest + corrective) out of the accumulators (1 / pscale rides in the rotation entries'
        // weights); into the exchange at the vertex's column.  (Packed FMAs -- two vertices an instruction -- measured: no faster.)
#define LX_APPLY(TT) { \
        unsigned fl_o = (unsigned)fl; LX_OPAQUE(fl_o);   /* (not a tile-loop invariant to be parked in a register: recomputed per block) */ \
        char* sx = Sx + ((TT) & 1) * LX_SXBYTES + fl_o * (LX_XP * 4); \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) { \
            const float px = acc[TT][0][r], py = acc[TT][1][r], pz = acc[TT][2][r]; \
            float* so = reinterpret_cast<float*>(sx + xo[r]); \
            _Pragma("unroll") for (int c = 0; c < 3; ++c) so[c] = fmaf(T[c][0][r], px, fmaf(T[c][1][r], py, fmaf(T[c][2][r], pz, T[c][3][r]))); \
        } }
#define LX_BLOCK(TT) { \
        constexpr int t = (TT); \
        __builtin_amdgcn_s_waitcnt(0x0F70); \
        __builtin_amdgcn_sched_barrier(0); \
        if (t >= 2) { LX_KEEP(rv[0]); LX_KEEP(rv[1]); LX_KEEP(rv[2]); } \
        LX_BLEND(w0s, w0, true) \
        __builtin_amdgcn_sched_barrier(0); \
        if (nr > 1) load_item(abase + (unsigned)t * tlb, (unsigned)ljt[LX_JR + q4] + (unsigned)fl * 48u); \
        else if (t < 7) load_item(abase + (unsigned)(t + 1) * tlb, off0); \
        __builtin_amdgcn_sched_barrier(0); \
        if (t == 3) LX_STAMP(16) \
        if (t >= 1) { row_read(t - 1); if (t == 3) LX_STAMP(17) row_write(t - 1, false); } \
        __builtin_amdgcn_sched_barrier(0); \
        if (t == 3) LX_STAMP(13) \
        for (int q = 1; q < nr; ++q) { \
            const float wq = *reinterpret_cast<const float*>(lds_raw + LX_OFF_W + ((wv * NRM + q) * 16 + fl) * 16 + q4 * 4); \
            const float wqs = wq * isc; \
            __builtin_amdgcn_s_waitcnt(0x0F70); __builtin_amdgcn_sched_barrier(0); \
            if (t >= 1) { LX_KEEP(rv[0]); LX_KEEP(rv[1]); LX_KEEP(rv[2]); } \
            LX_BLEND(wqs, wq, false) \
            __builtin_amdgcn_sched_barrier(0); \
            if (q + 1 < nr) load_item(abase + (unsigned)t * tlb, (unsigned)ljt[(q + 1) * LX_JR + q4] + (unsigned)fl * 48u); \
            else if (t < 7) load_item(abase + (unsigned)(t + 1) * tlb, off0); \
            __builtin_amdgcn_sched_barrier(0); \
        } \
        if (t == 3) LX_STAMP(14) \
        LX_APPLY(TT) \
        if (t == 3) LX_STAMP(15) \
        LBS_LDS_BARRIER(); \
        LX_STAMP(3 + t) }
        // (A branch-free variant of the block for one-round groups on interior tiles -- the same steps as straight-line code, ~60 instructions
        //  instead of ~75 and a dozen scalar branches -- was measured slower, 170-178 against 151 us per call, with and without spills in
        //  its steady state, with counted or full waits: not kept.  Where in the block the previous block's rows are read and stored --
        //  behind the matrix instructions, behind the apply, or the read ahead of them -- makes no difference: 149-154 us all three.)
        LX_BLOCK(0) LX_BLOCK(1) LX_BLOCK(2) LX_BLOCK(3) LX_BLOCK(4) LX_BLOCK(5) LX_BLOCK(6) LX_BLOCK(7)
#undef LX_APPLY
#undef LX_BLEND
#undef LX_BLOCK
        __builtin_amdgcn_s_waitcnt(0x0F70); LX_KEEP(rv[0]); LX_KEEP(rv[1]); LX_KEEP(rv[2]);
        row_read(7);
        row_write(7, true);
        LX_STAMP(11)
    }
    if ((dbg & 32) && dbgbuf != nullptr && tid == 0 && blockIdx.x < 512) {
        dbgbuf[blockIdx.x * 2] = wg_t0;
        dbgbuf[blockIdx.x * 2 + 1] = wall_clock64();
    }
#undef LX_LD_G
#undef LX_ST_G
#undef LX_LD_A
#undef LX_LD_B
#undef LX_LD_B1
#undef LX_MMA_T
#undef LX_STEP
#undef LX_STAMP
}

// ---- vertex normals of exported meshes (moshii_vertex_normals_*, moshii_virtual_markers_*) ----------------------------------------
// VertNormals(normalized=True) (reference src/moshpp/models/ch_vert_normals.py; psbody estimate_vertex_normals): the unnormalised
// cross products of a vertex's incident faces summed, divided by the length of the sum; a zero sum gives (0, 0, 0).
// The faces come as a vertex -> incident-corner table in CSR form (moshii_model_set_faces): rows[v] .. rows[v + 1] index `pairs`, one
// entry per incident face = the two other vertices (p, q) in the face's cyclic order, so the face's scaled normal is
// (p - v) x (q - v).  Entries are 16-bit pairs in one dword while V <= 65 535 (W16; SMPL-H: 183 KB, read once per frame, L2
// resident), two dwords otherwise.
// Four lanes (a quad) share a vertex: lane `sub` takes corners sub, sub + 4, ... of the row, the partial sums meet through two
// DPP quad permutes -- valence runs from 5 to 34 on these bodies, and a wave waits for its longest row: a quarter of it this way --
// and lanes 0 .. 2 of the quad store x, y, z: a wave writes 16 consecutive vertices, 192 contiguous bytes.
// Arithmetic in VN_ACC_T = double for both precisions (the f32 call converts its inputs and rounds once on the store): f32 cross
// products lose up to 5.6e-7 on sliver triangles.  (Frame sizes below are those of the released bodies: SMPL-H V = 6 890, SMPL-X
// V = 10 475; the triangulated synthetic bodies of the tests and of tools/lbs_bench.py --normals are larger: 7 634 / 11 270.)  -DVN_ACC_T=float builds the f32-accumulating kernel for timing comparisons only.
#ifndef VN_ACC_T
#define VN_ACC_T double
#endif
#define VN_THREADS 1024                 // k_vn_lds: 16 waves = 256 quads
#define VN_LDS_MAX (160 * 1024 - 256)   // a workgroup's frames in LDS (SMPL-H 82.7 KB, SMPL-X 125.7 KB a frame)
#define VN_LDS_PAIR (78 * 1024)         // small bodies: as many frames as keep TWO workgroups on a CU (one loads while the other computes)

template <int CTRL>
__device__ __forceinline__ double vn_dpp(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float vn_dpp(float x) {
    int b;
    __builtin_memcpy(&b, &x, 4);
    b = __builtin_amdgcn_update_dpp(0, b, CTRL, 0xf, 0xf, false);
    __builtin_memcpy(&x, &b, 4);
    return x;
}
// sum over the four lanes of a quad, the same bits in all four (quad_perm [1,0,3,2], then [2,3,0,1])
template <class A>
__device__ __forceinline__ A vn_quad_sum(A x) {
    x += vn_dpp<0xB1>(x);
    x += vn_dpp<0x4E>(x);
    return x;
}

// lane `sub` of a quad: its share of vertex v's row on the mesh `fr` ([V][3], LDS or global), summed over the quad and normalised.
// EVERY lane of the wave calls this (the quad permutes are wave-wide); `valid` = false lanes read nothing.
template <class A, class T, bool W16>
__device__ __forceinline__ void vn_vertex(const T* fr, unsigned v, int sub, bool valid, const unsigned* __restrict__ rows,
                                          const unsigned* __restrict__ pairs, A* n, A* pos) {
    A sx = 0, sy = 0, sz = 0, vx = 0, vy = 0, vz = 0;
    if (valid) {
        const unsigned beg = rows[v], end = rows[v + 1];
        vx = (A)fr[3 * v]; vy = (A)fr[3 * v + 1]; vz = (A)fr[3 * v + 2];
        for (unsigned c = beg + sub; c < end; c += 4) {
            unsigned p, q;
            if (W16) { const unsigned w = pairs[c]; p = w & 0xffffu; q = w >> 16; }
            else { p = pairs[2 * (size_t)c]; q = pairs[2 * (size_t)c + 1]; }
            const A ax = (A)fr[3 * p] - vx, ay = (A)fr[3 * p + 1] - vy, az = (A)fr[3 * p + 2] - vz;
            const A bx = (A)fr[3 * q] - vx, by = (A)fr[3 * q + 1] - vy, bz = (A)fr[3 * q + 2] - vz;
            sx += ay * bz - az * by;
            sy += az * bx - ax * bz;
            sz += ax * by - ay * bx;
        }
    }
    sx = vn_quad_sum(sx); sy = vn_quad_sum(sy); sz = vn_quad_sum(sz);
    const A d = sx * sx + sy * sy + sz * sz;
    const A inv = d > (A)0 ? (A)1 / (A)sqrt((double)d) : (A)0;
    n[0] = sx * inv; n[1] = sy * inv; n[2] = sz * inv;
    pos[0] = vx; pos[1] = vy; pos[2] = vz;
}

// f32 hot path: a workgroup takes G whole frames at a time.  The frames' G x V x 12 bytes go to LDS with 16-byte loads (the LDS copy
// starts `a` floats in, a = the global address's dword offset within 16 bytes, so that both sides of every 16-byte move are aligned;
// up to three floats at either end move alone), the quads walk the CSR rows and gather the neighbours from LDS.
template <bool W16>
__global__ __launch_bounds__(VN_THREADS) void k_vn_lds(int V, int F, int G, const float* __restrict__ verts, float* __restrict__ normals,
                                                        const unsigned* __restrict__ rows, const unsigned* __restrict__ pairs) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    const int tid = threadIdx.x, sub = tid & 3;
    const unsigned fv = (unsigned)V * 3;
    for (int fb = blockIdx.x * G; fb < F; fb += gridDim.x * G) {
        const int ng = min(G, F - fb);
        const float* src = verts + (size_t)fb * fv;
        const unsigned n = (unsigned)ng * fv;
        const unsigned a = (unsigned)(((size_t)src >> 2) & 3), head = ((4u - a) & 3u) < n ? ((4u - a) & 3u) : n, n4 = (n - head) >> 2, tail = n - head - 4 * n4;
        for (unsigned i = tid; i < n4; i += VN_THREADS)
            *reinterpret_cast<f32x4*>(smf + a + head + 4 * i) = *reinterpret_cast<const f32x4*>(src + head + 4 * i);
        if ((unsigned)tid < head) smf[a + tid] = src[tid];
        if ((unsigned)tid < tail) smf[a + head + 4 * n4 + tid] = src[head + 4 * n4 + tid];
        __syncthreads();
        for (int fl = 0; fl < ng; ++fl) {
            const float* fr = smf + a + (unsigned)fl * fv;
            float* out = normals + (size_t)(fb + fl) * fv;
            for (unsigned v0 = 0; v0 < (unsigned)V; v0 += VN_THREADS / 4) {
                const unsigned v = v0 + (tid >> 2);
                VN_ACC_T nr[3], pos[3];
                vn_vertex<VN_ACC_T, float, W16>(fr, v, sub, v < (unsigned)V, rows, pairs, nr, pos);
                if (v < (unsigned)V && sub < 3) out[3 * v + sub] = (float)(sub == 0 ? nr[0] : sub == 1 ? nr[1] : nr[2]);
            }
        }
        __syncthreads();
    }
}

// The same rows with the neighbours gathered through L2: the f64 call (an f64 SMPL-H frame is 165 KB), f32 frames beyond the LDS
// budget, MOSHII_VN_KERNEL=gather.  A workgroup = 64 consecutive vertices, walked over the frames blockIdx.y, + gridDim.y, ...
template <class T, bool W16>
__global__ __launch_bounds__(256) void k_vn_gather(int V, int F, const T* __restrict__ verts, T* __restrict__ normals,
                                                    const unsigned* __restrict__ rows, const unsigned* __restrict__ pairs) {
    typedef typename std::conditional<std::is_same<T, double>::value, double, VN_ACC_T>::type A;
    const int tid = threadIdx.x, sub = tid & 3;
    const unsigned fv = (unsigned)V * 3, v = blockIdx.x * 64 + (tid >> 2);
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
        A nr[3], pos[3];
        vn_vertex<A, T, W16>(verts + (size_t)f * fv, v, sub, v < (unsigned)V, rows, pairs, nr, pos);
        if (v < (unsigned)V && sub < 3) normals[(size_t)f * fv + 3 * v + sub] = (T)(sub == 0 ? nr[0] : sub == 1 ? nr[1] : nr[2]);
    }
}

// Virtual markers of a batch of meshes: marker i of frame f = verts[f][vids[i]] + dist[i] x its vertex normal -- the reference's
// prepare_mosh_markers_latent (src/moshpp/chmosh.py:57-67) on every frame.  One quad per (frame, marker), f64 arithmetic in both
// precisions; only the M rows of the marker vertices are walked.
template <class T, bool W16>
__global__ __launch_bounds__(256) void k_vn_markers(int V, int nf, int M, const T* __restrict__ verts, const int* __restrict__ vids,
                                                     const double* __restrict__ dist, T* __restrict__ markers, T* __restrict__ mnormals,
                                                     const unsigned* __restrict__ rows, const unsigned* __restrict__ pairs) {
    const int tid = threadIdx.x, sub = tid & 3;
    const unsigned total = (unsigned)nf * (unsigned)M, item = blockIdx.x * 64 + (tid >> 2);
    const bool valid = item < total;
    const unsigned f = valid ? item / (unsigned)M : 0, i = valid ? item - f * (unsigned)M : 0;
    double nr[3], pos[3];
    vn_vertex<double, T, W16>(verts + (size_t)f * V * 3, valid ? (unsigned)vids[i] : 0u, sub, valid, rows, pairs, nr, pos);
    if (valid && sub < 3) {
        const double nc = sub == 0 ? nr[0] : sub == 1 ? nr[1] : nr[2], pc = sub == 0 ? pos[0] : sub == 1 ? pos[1] : pos[2];
        markers[(size_t)item * 3 + sub] = (T)(pc + dist[i] * nc);
        if (mnormals) mnormals[(size_t)item * 3 + sub] = (T)nc;
    }
}

// ---- signed point-to-mesh distance of posed meshes (moshii_surface_distance_*, moshii_marker_surface_distance_*) ----
// The reference's PtsToMesh(signed=True) (scan2mesh/mesh_distance_main.py:158-297) for every point of every frame, exhaustive over the
// triangles: nearest triangle by the region tests of closest_on_tri (stagei.hip) / the oracle's _closest_on_triangles, ties to the
// lowest face id, sign from (p - nearest) . n with n the face normal (interior), the vertex normal (vertex) or the sum of the two
// vertex normals (edge).  Two steps:
//   search   k_sd_lds / k_sd_gather: a wave takes SD_PB points of one frame, its lanes deal the triangles among themselves, every
//            lane keeps (d^2, face id) per point in the call's precision, and the wave's lexicographic minimum (shuffles) is the
//            winner: d^2 first, then the id, so no order of arrival decides a tie.  Only the winner's id leaves the search.
//   finish   k_sd_finish: one quad per point evaluates the winner once in f64 from the inputs as given (closest point, part, the
//            part's normals through the CSR rows of the normals kernels, sign, distance) and rounds once on the store.
// Every product of the search is taken between DIFFERENCES of the inputs (b - a, c - a, p - a; the residual p - q = ap - s ab - t ac),
// so its error scales with the distances involved, not with where the frame stands: the frames are staged as they are, uncentred.
// All of it in explicit fma / single operations: the two f32 searches give the same d^2 bits for a (point, triangle) whatever the
// compiler contracts elsewhere, hence the same winners.
#define SD_THREADS 1024                  // k_sd_lds: 16 waves
#define SD_NOFACE 0x7fffffff

__device__ __forceinline__ float sd_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double sd_rcp(double x) { return 1.0 / x; }
__device__ __forceinline__ float sd_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double sd_fma(double a, double b, double c) { return fma(a, b, c); }
template <class T>
__device__ __forceinline__ T sd_dot(const T* a, const T* b) { return sd_fma(a[2], b[2], sd_fma(a[1], b[1], a[0] * b[0])); }

// closest point of the triangle (a, a + ab, a + ac) to a + ap as q = a + s ab + t ac; returns the part code (0 interior, 1 ab, 2 bc,
// 3 ca, 4 a, 5 b, 6 c) by the oracle's order of tests.  e00 = ab.ab, e01 = ab.ac, e11 = ac.ac.  A triangle without area gives NaN.
template <class T>
__device__ __forceinline__ int sd_closest(const T* ab, const T* ac, T e00, T e01, T e11, const T* ap, T* s, T* t) {
    const T d1 = sd_dot(ab, ap), d2 = sd_dot(ac, ap);
    const T d3 = d1 - e00, d4 = d2 - e01, d5 = d1 - e01, d6 = d2 - e11;     // ab.bp, ac.bp, ab.cp, ac.cp
    const T vc = sd_fma(d1, d4, -(d3 * d2)), vb = sd_fma(d5, d2, -(d1 * d6)), va = sd_fma(d3, d6, -(d5 * d4));
    const T d43 = d4 - d3, d56 = d5 - d6;
    const int part = (d1 <= 0 && d2 <= 0) ? 4 : (d3 >= 0 && d4 <= d3) ? 5 : (vc <= 0 && d1 >= 0 && d3 <= 0) ? 1 : (d6 >= 0 && d5 <= d6) ? 6
                   : (vb <= 0 && d2 >= 0 && d6 <= 0) ? 3 : (va <= 0 && d43 >= 0 && d56 >= 0) ? 2 : 0;
    const T den = part == 1 ? d1 - d3 : part == 3 ? d2 - d6 : part == 2 ? d43 + d56 : part == 0 ? (va + vb) + vc : (T)1;
    const T r = sd_rcp(den);
    const T u = d43 * r;                                                     // (part 2: q = b + u (c - b))
    *s = part == 5 ? (T)1 : part == 1 ? d1 * r : part == 2 ? (T)1 - u : part == 0 ? vb * r : (T)0;
    *t = part == 6 ? (T)1 : part == 3 ? d2 * r : part == 2 ? u : part == 0 ? vc * r : (T)0;
    return part;
}

__device__ __forceinline__ void sd_face_ids(const unsigned* __restrict__ tris, bool w16, unsigned f, unsigned* ia, unsigned* ib, unsigned* ic) {
    if (w16) {   // four 16-bit fields a face (the fourth unused): one 8-byte load
        const unsigned long long w = reinterpret_cast<const unsigned long long*>(tris)[f];
        *ia = (unsigned)w & 0xffffu; *ib = ((unsigned)w >> 16) & 0xffffu; *ic = (unsigned)(w >> 32) & 0xffffu;
    }
    else { *ia = tris[3 * (size_t)f]; *ib = tris[3 * (size_t)f + 1]; *ic = tris[3 * (size_t)f + 2]; }
}

// One wave: the nearest triangle of each of the np <= PB points pts[0 .. np) (x, y, z apiece) on the mesh fr ([V][3], LDS or global),
// written to win[0 .. np) by lane 0: SD_NOFACE for an absent point (a non-finite coordinate: it costs no test) and where no triangle
// has a distance.  EVERY lane of the wave calls this.
template <class T, int PB, bool W16>
__device__ __forceinline__ void sd_search(const T* fr, int NF, const unsigned* __restrict__ tris, const T* __restrict__ pts, int np, int lane, int* win) {
    T p[PB][3], best[PB];
    int bid[PB];
    bool any = false;
#pragma unroll
    for (int k = 0; k < PB; ++k) {
        bool ok = k < np;
        for (int i = 0; i < 3; ++i) { p[k][i] = ok ? pts[3 * k + i] : (T)0; ok = ok && p[k][i] - p[k][i] == (T)0; }   // (x - x: NaN for NaN and the infinities)
        // (an absent point keeps a NaN coordinate: its d^2 is NaN and never passes `<`)
        if (!ok) p[k][0] = (T)NAN;
        any = any || ok;
        best[k] = (T)INFINITY; bid[k] = SD_NOFACE;
    }
    if (any)
        for (int f = lane; f < NF; f += 64) {
            unsigned ia, ib, ic;
            sd_face_ids(tris, W16, (unsigned)f, &ia, &ib, &ic);
            if (ia == ib || ib == ic || ia == ic) continue;               // a face that names a vertex twice never wins
            T a[3], ab[3], ac[3];
            for (int i = 0; i < 3; ++i) { a[i] = fr[3 * ia + i]; ab[i] = fr[3 * ib + i] - a[i]; ac[i] = fr[3 * ic + i] - a[i]; }
            const T e00 = sd_dot(ab, ab), e01 = sd_dot(ab, ac), e11 = sd_dot(ac, ac);
            // the triangle's normal: (s, t) are solved for the point's FOOT on the plane, ap - h n, so that the dot products the region
            // tests multiply stay as small as the in-plane offsets -- a point a metre off a centimetre triangle would otherwise lose
            // the digits its coefficients live in.  The residual below is taken from ap itself.
            const T n[3] = {sd_fma(ab[1], ac[2], -(ab[2] * ac[1])), sd_fma(ab[2], ac[0], -(ab[0] * ac[2])), sd_fma(ab[0], ac[1], -(ab[1] * ac[0]))};
            const T nn = sd_dot(n, n), rn = nn > (T)0 ? sd_rcp(nn) : (T)0;
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                T ap[3], apl[3], s, t, df[3];
                for (int i = 0; i < 3; ++i) ap[i] = p[k][i] - a[i];
                const T h = sd_dot(ap, n) * rn;
                for (int i = 0; i < 3; ++i) apl[i] = sd_fma(-h, n[i], ap[i]);
                const int part = sd_closest(ab, ac, e00, e01, e11, apl, &s, &t);
                for (int i = 0; i < 3; ++i) df[i] = sd_fma(-t, ac[i], sd_fma(-s, ab[i], ap[i]));
                // above the interior the distance is the height alone: (s, t) of a thin triangle would add an in-plane residual
                const T dd = part == 0 ? h * h * nn : sd_dot(df, df);
                if (dd < best[k]) { best[k] = dd; bid[k] = f; }           // (a lane's ids ascend: `<` keeps its lowest on a tie)
            }
        }
#pragma unroll
    for (int k = 0; k < PB; ++k) {
        if (any)
            for (int off = 32; off > 0; off >>= 1) {
                const T od = __shfl_down(best[k], off);
                const int oi = __shfl_down(bid[k], off);
                if (od < best[k] || (od == best[k] && oi < bid[k])) { best[k] = od; bid[k] = oi; }
            }
        if (lane == 0 && k < np) win[k] = bid[k];
    }
}

// The staged f32 search (MOSHII_SD_KERNEL=lds; not the default, see moshii_launch_surface_distance): a workgroup keeps G whole frames in LDS (the copy of k_vn_lds), its 16 waves take the (frame, group of PB points)
// pairs in turn; the face table is the same for every frame and comes through L2.
template <int PB, bool W16>
__global__ __launch_bounds__(SD_THREADS) void k_sd_lds(int V, int NF, int F, int G, int N, const float* __restrict__ verts,
                                                        const float* __restrict__ points, const unsigned* __restrict__ tris, int* __restrict__ win) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned fv = (unsigned)V * 3;
    const int ngrp = (N + PB - 1) / PB;
    for (int fb = blockIdx.x * G; fb < F; fb += gridDim.x * G) {
        const int ng = min(G, F - fb);
        const float* src = verts + (size_t)fb * fv;
        const unsigned n = (unsigned)ng * fv;
        const unsigned a = (unsigned)(((size_t)src >> 2) & 3), head = ((4u - a) & 3u) < n ? ((4u - a) & 3u) : n, n4 = (n - head) >> 2, tail = n - head - 4 * n4;
        for (unsigned i = tid; i < n4; i += SD_THREADS)
            *reinterpret_cast<f32x4*>(smf + a + head + 4 * i) = *reinterpret_cast<const f32x4*>(src + head + 4 * i);
        if ((unsigned)tid < head) smf[a + tid] = src[tid];
        if ((unsigned)tid < tail) smf[a + head + 4 * n4 + tid] = src[head + 4 * n4 + tid];
        __syncthreads();
        for (int it = wave; it < ng * ngrp; it += SD_THREADS / 64) {
            const int fl = it / ngrp, g = it - fl * ngrp;
            const size_t at = (size_t)(fb + fl) * N + (size_t)g * PB;
            sd_search<float, PB, W16>(smf + a + (unsigned)fl * fv, NF, tris, points + 3 * at, min(PB, N - g * PB), lane, win + at);
        }
        __syncthreads();
    }
}

// The same search with the vertices read through L2: the default of both precisions.
// A workgroup = 4 waves, a wave per (frame, group of PB points), walked with the grid's stride.
template <class T, int PB, bool W16>
__global__ __launch_bounds__(256) void k_sd_gather(int V, int NF, long long F, int N, const T* __restrict__ verts, const T* __restrict__ points,
                                                    const unsigned* __restrict__ tris, int* __restrict__ win) {
    const int lane = threadIdx.x & 63;
    const long long ngrp = (N + PB - 1) / PB, items = F * ngrp;
    for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
        const long long f = it / ngrp;
        const int g = (int)(it - f * ngrp);
        const size_t at = (size_t)f * N + (size_t)g * PB;
        sd_search<T, PB, W16>(verts + (size_t)f * V * 3, NF, tris, points + 3 * at, min(PB, N - g * PB), lane, win + at);
    }
}

// The winners in f64, one quad per point: total = F x N points, face[] holds the search's winner on entry and the face id (or -1)
// on return; part / nearest may be null.
template <class T, bool W16>
__global__ __launch_bounds__(256) void k_sd_finish(int V, long long total, int N, const T* __restrict__ verts, const T* __restrict__ points,
                                                    const unsigned* __restrict__ tris, const unsigned* __restrict__ rows,
                                                    const unsigned* __restrict__ pairs, T* __restrict__ dist, int* face, int* __restrict__ part,
                                                    T* __restrict__ nearest) {
    const int tid = threadIdx.x, sub = tid & 3;
    for (long long i0 = (long long)blockIdx.x * 64; i0 < total; i0 += (long long)gridDim.x * 64) {
        const long long item = i0 + (tid >> 2);
        const bool in = item < total;
        const int w = in ? face[item] : SD_NOFACE;
        const bool found = in && w != SD_NOFACE;
        const T* fr = verts + (size_t)(in ? item / N : 0) * V * 3;
        double p[3] = {0, 0, 0}, a[3] = {0, 0, 0}, ab[3] = {0, 0, 0}, ac[3] = {0, 0, 0}, ap[3], s = 0, t = 0;
        unsigned id[3] = {0, 0, 0};
        int pc = -1;
        if (found) {
            sd_face_ids(tris, W16, (unsigned)w, &id[0], &id[1], &id[2]);
            for (int i = 0; i < 3; ++i) {
                p[i] = (double)points[(size_t)item * 3 + i];
                a[i] = (double)fr[3 * (size_t)id[0] + i];
                ab[i] = (double)fr[3 * (size_t)id[1] + i] - a[i];
                ac[i] = (double)fr[3 * (size_t)id[2] + i] - a[i];
            }
            for (int i = 0; i < 3; ++i) ap[i] = p[i] - a[i];
            pc = sd_closest(ab, ac, sd_dot(ab, ab), sd_dot(ab, ac), sd_dot(ac, ac), ap, &s, &t);
        }
        // the normals of the part: none (interior), one vertex, or the two ends of an edge -- the quad walks their rows together
        const bool one = found && pc > 0;
        const bool two = found && pc > 0 && pc <= 3;
        const int k0 = pc > 3 ? pc - 4 : pc - 1, k1 = pc % 3;
        const unsigned v0 = one ? (k0 == 0 ? id[0] : k0 == 1 ? id[1] : id[2]) : 0u, v1 = two ? (k1 == 0 ? id[0] : k1 == 1 ? id[1] : id[2]) : 0u;
        double n0[3], n1[3], pos[3];
        vn_vertex<double, T, W16>(fr, v0, sub, one, rows, pairs, n0, pos);
        vn_vertex<double, T, W16>(fr, v1, sub, two, rows, pairs, n1, pos);
        if (!in || sub != 0) continue;
        if (!found) {
            dist[item] = (T)NAN; face[item] = -1;
            if (part) part[item] = -1;
            if (nearest) for (int i = 0; i < 3; ++i) nearest[(size_t)item * 3 + i] = (T)NAN;
            continue;
        }
        double df[3], q[3], nn[3];
        for (int i = 0; i < 3; ++i) {
            const double off = sd_fma(t, ac[i], s * ab[i]);
            q[i] = a[i] + off; df[i] = ap[i] - off;
        }
        if (pc == 0) { nn[0] = ab[1] * ac[2] - ab[2] * ac[1]; nn[1] = ab[2] * ac[0] - ab[0] * ac[2]; nn[2] = ab[0] * ac[1] - ab[1] * ac[0]; }
        else for (int i = 0; i < 3; ++i) nn[i] = two ? n0[i] + n1[i] : n0[i];
        const double sd = sd_dot(df, nn);
        const double dir = sd > 0 ? 1.0 : sd < 0 ? -1.0 : 0.0;
        dist[item] = (T)(sqrt(sd_dot(df, df)) * dir);
        if (part) part[item] = pc;
        if (nearest) for (int i = 0; i < 3; ++i) nearest[(size_t)item * 3 + i] = (T)q[i];
    }
}

// ---- posed joints and world joint rotations of solved frames (moshii_joints_*) ----------------------------------------------------
// The reference's J_transformed / A_global (src/moshpp/models/smpl_fast_derivatives.py:218-229) for F frames: the kinematic chain
// alone, no vertex touched.  K <= 64 joints are exactly one wavefront: ONE WAVE PER FRAME, LANE k = JOINT k, JT_WAVES frames a
// workgroup, no loop over frames.  Everything of a frame lives in the wave's registers, in f64 whatever T is (T = float converts on
// the loads and rounds once on the stores):
//   fullpose   the lane's three components: the pose variables themselves (body joints) or hands_mean + sum_i pose_hand[i] comps[i][h]
//              over each column's non-zero rows col_lo .. col_hi, the rows of the lane's three columns fetched JT_ROWS at a time
//   Rodrigues  the evaluation of k_lbs_f64 (moshii_api.hip), term for term: joints and exported vertices describe the same body
//   joints     SH: J_k + JS[k] . shape[f], summed in k_lbs_f64's order
//   chain      level by level: at depth d the lanes of that depth take their parent's world rotation and position ACROSS LANES (twelve
//              f64 shuffles a level, every lane taking part in each: the loop bound maxdepth is uniform) and form Rw = Rw_p . R,
//              tw = Rw_p . (J_k - J_p) + tw_p in k_lbs_f64's order of operations.  No LDS, no barrier.
// A wave's output is one contiguous run: lane k stores its 3 (and 9) values behind lane k - 1's.  Waves behind the last frame and lanes
// behind the last joint shadow frame F - 1 / joint K - 1 and store nothing.  All addressing is 64-bit.
#define JT_WAVES 4
#define JT_ROWS 8              // hand-component rows a lane fetches in one batch
template <class T, bool SH>
__global__ __launch_bounds__(64 * JT_WAVES) void k_joints(ModelDev md, int F, const T* __restrict__ pose, const T* __restrict__ trans,
                                                          const T* __restrict__ shape, T* __restrict__ joints, T* __restrict__ rot) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, K = md.K;
    const long long fw = (long long)blockIdx.x * JT_WAVES + wv;
    const size_t f = (size_t)(fw < F ? fw : F - 1);
    const int k = lane < K ? lane : K - 1;
    const bool act = lane < K && fw < F;
    const int p = md.parents[k], dk = lane < K ? md.depth[k] : -1;
    const T* ps = pose + f * md.NP;
    const int bd = md.body_dof, nhf = md.nhand_full;
    double rv[3], Jk[3];
    if (3 * k < bd) {                // (body_dof is a multiple of three: a joint's components are pose variables or hand dofs together)
#pragma unroll
        for (int i = 0; i < 3; ++i) rv[i] = (double)ps[3 * k + i];
    } else {
        // component i sums its own rows lo[i] .. hi[i] in ascending order; the rows of all three are fetched together, JT_ROWS at a time (one
        // round trip a batch instead of one a row and component: what a wave waits for here is latency)
        const int h = 3 * k - bd;
        int lo[3], hi[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { lo[i] = md.col_lo[h + i]; hi[i] = md.col_hi[h + i]; rv[i] = md.hands_mean[h + i]; }
        const int c0 = min(min(lo[0], lo[1]), lo[2]), c1 = max(max(hi[0], hi[1]), hi[2]);
        for (int c = c0; c < c1; c += JT_ROWS) {
            double pu[JT_ROWS], cm[JT_ROWS][3];
#pragma unroll
            for (int u = 0; u < JT_ROWS; ++u) {
                const int cc = min(c + u, c1 - 1);
                pu[u] = (double)ps[bd + cc];
#pragma unroll
                for (int i = 0; i < 3; ++i) cm[u][i] = md.comps[(size_t)cc * nhf + h + i];
            }
#pragma unroll
            for (int u = 0; u < JT_ROWS; ++u)
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (c + u >= lo[i] && c + u < hi[i]) rv[i] += pu[u] * cm[u][i];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int d = 3 * k + i;
        double s = md.J[d];
        if (SH) {
            const int E = md.nshape;
            const T* cf = shape + f * E;
#pragma unroll 4
            for (int e = 0; e < E; ++e) s += md.JS[((size_t)k * E + e) * 3 + i] * (double)cf[e];
        }
        Jk[i] = s;
    }
    double R[9];
    {
        const double x = rv[0], y = rv[1], z = rv[2];
        const double t2 = x * x + y * y + z * z;
        double a, b;
        if (t2 < 1e-6) { a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0; b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0; }
        else { const double t = sqrt(t2); a = sin(t) / t; b = (1.0 - cos(t)) / t2; }
        const double K2[9] = {x * x - t2, x * y, x * z, x * y, y * y - t2, y * z, x * z, y * z, z * z - t2};
        const double Km[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0) + a * Km[e] + b * K2[e];
    }
    // the root's world transform is its own; every other lane's is formed at its depth
    double Rw[9], tw[3], dJ[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rw[e] = R[e];
    const int src = p > 0 ? p : 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) { tw[i] = Jk[i]; dJ[i] = Jk[i] - __shfl(Jk[i], src); }
    for (int d = 1; d <= md.maxdepth; ++d) {
        double pr[9], pt[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) pr[e] = __shfl(Rw[e], src);
#pragma unroll
        for (int i = 0; i < 3; ++i) pt[i] = __shfl(tw[i], src);
        if (dk == d) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) Rw[i * 3 + j] = pr[i * 3 + 0] * R[0 * 3 + j] + pr[i * 3 + 1] * R[1 * 3 + j] + pr[i * 3 + 2] * R[2 * 3 + j];
                tw[i] = pr[i * 3 + 0] * dJ[0] + pr[i * 3 + 1] * dJ[1] + pr[i * 3 + 2] * dJ[2] + pt[i];
            }
        }
    }
    if (!act) return;
    const T* tr = trans + f * 3;
    T* oj = joints + (f * K + k) * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) oj[i] = (T)(tw[i] + (double)tr[i]);
    if (rot != nullptr) {
        T* orot = rot + (f * K + k) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) orot[e] = (T)Rw[e];
    }
}

// ---- shaded previews of exported meshes (moshii_render_*, moshii_render_posed_*) --------------------------------------------------
// What the reference shows while it solves (tools/visualization.py:96-130: the body with observed and simulated markers), rasterised
// here by the rules of include/moshii.h ("Rendering rules"): pinhole camera in f64, screen positions snapped to a 1/16-pixel grid,
// integer edge functions with the top-left rule, perspective-correct depth rounded once to f32, smallest depth wins, ties to the
// lower id, markers as camera-facing discs, headlight shading.  Two kernels:
//   k_render_project<T>  per (frame, vertex): camera-space depth, snapped position, camera-space normal -> one 32-byte RenderVertex;
//                        per (frame, marker): centre, half axes, depth -> one RenderMarker.  The only kernel that reads T.
//   k_render_tiles       ONE WORKGROUP OF 1024 LANES OWNS ONE 32 x 32 TILE OF ONE FRAME, one lane one pixel, the pixel's best
//                        (depth, id) in the lane's registers.  Nothing is ever written to the image but the owner's final store: no
//                        atomics on the image, so no order of arrival exists and two runs give the same bits.
// The workgroup walks the items (faces 0 .. NF - 1, then markers NF .. NF + N - 1) RD_CHUNK at a time: every lane takes one item, tests
// its snapped bounding box against the tile's pixel centres, and the survivors are compacted into an LDS list (ballot + popcount prefix
// within the wave, one LDS atomicAdd a wave for the wave's base: the list's order is arbitrary, the tie rule makes it irrelevant).  The
// lane that found a survivor also writes its set-up, once per tile: the three edge functions at the tile's first pixel centre (int64,
// the fill-rule bias folded in), their steps per pixel, and q_k = 1 / (z_k area2), so that a covered pixel's depth is
// 1 / (E_0 q_0 + E_1 q_1 + E_2 q_2).  After a barrier every lane runs the list; all lanes read the same entry (an LDS broadcast).
// LDS: 76 bytes an entry in four arrays, 77 840 bytes for 1024 entries + the two counters: two workgroups would fit the 160 KB of a CU;
// at 76 VGPRs (6 waves a SIMD, a workgroup takes 4) the registers admit one.
// A body far away (all faces in one tile) costs NF / 1024 chunks of 1024 entries in that one workgroup; a few huge triangles cost one
// short list in every workgroup.  The lanes of a partial tile outside the image take part in everything but the final store.
#define RD_TILE 32
#define RD_THREADS (RD_TILE * RD_TILE)
#define RD_CHUNK 1024
#define RD_LDS_BYTES (RD_CHUNK * 76 + 16)
#define RD_SNAP_MAX 16777216.0   // 2^24

// X_c = R X + t, row major, summed left to right
__device__ __forceinline__ void rd_to_camera(const moshii_camera& c, double x, double y, double z, double* o) {
#pragma clang fp contract(off)
    o[0] = c.R[0] * x + c.R[1] * y + c.R[2] * z + c.t[0];
    o[1] = c.R[3] * x + c.R[4] * y + c.R[5] * z + c.t[1];
    o[2] = c.R[6] * x + c.R[7] * y + c.R[8] * z + c.t[2];
}
__device__ __forceinline__ bool rd_finite(double x) { return x - x == 0.0; }

template <class T>
__global__ __launch_bounds__(256) void k_render_project(int V, int N, int nf, int cam_stride, const moshii_camera* __restrict__ cams,
                                                        const T* __restrict__ verts, const T* __restrict__ normals,
                                                        const T* __restrict__ points, const double* __restrict__ radius,
                                                        RenderVertex* __restrict__ rec, RenderMarker* __restrict__ mrec) {
#pragma clang fp contract(off)
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= V + N) return;
    for (int f = blockIdx.y; f < nf; f += gridDim.y) {
        const moshii_camera& c = cams[(size_t)f * cam_stride];
        if (item < V) {
            const T* p = verts + ((size_t)f * V + item) * 3;
            const T* n = normals + ((size_t)f * V + item) * 3;
            double xc[3];
            rd_to_camera(c, (double)p[0], (double)p[1], (double)p[2], xc);
            RenderVertex r;
            r.sx = 0; r.sy = 0; r.z = xc[2]; r.ok = 0;
            const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
            r.n[0] = (float)(c.R[0] * nx + c.R[1] * ny + c.R[2] * nz);
            r.n[1] = (float)(c.R[3] * nx + c.R[4] * ny + c.R[5] * nz);
            r.n[2] = (float)(c.R[6] * nx + c.R[7] * ny + c.R[8] * nz);
            if (rd_finite(xc[0]) && rd_finite(xc[1]) && rd_finite(xc[2]) && xc[2] > c.znear) {
                const double u = c.fx * xc[0] / xc[2] + c.cx, v = c.fy * xc[1] / xc[2] + c.cy;
                const double su = floor(16.0 * u + 0.5), sv = floor(16.0 * v + 0.5);
                if (rd_finite(su) && rd_finite(sv) && fabs(su) <= RD_SNAP_MAX && fabs(sv) <= RD_SNAP_MAX) { r.sx = (int)su; r.sy = (int)sv; r.ok = 1; }
            }
            rec[(size_t)f * V + item] = r;
        } else {
            const int k = item - V;
            const T* p = points + ((size_t)f * N + k) * 3;
            const double rad = radius[k];
            double xc[3];
            rd_to_camera(c, (double)p[0], (double)p[1], (double)p[2], xc);
            RenderMarker m;
            m.uc = 0.0; m.vc = 0.0; m.rx = 0.0; m.ry = 0.0; m.depth = 0.0f; m.ok = 0;
            if (rd_finite(xc[0]) && rd_finite(xc[1]) && rd_finite(xc[2]) && rad > 0.0 && xc[2] - rad > c.znear) {
                m.uc = c.fx * xc[0] / xc[2] + c.cx; m.vc = c.fy * xc[1] / xc[2] + c.cy;
                m.rx = c.fx * rad / xc[2]; m.ry = c.fy * rad / xc[2];
                m.depth = (float)(xc[2] - rad);
                m.ok = rd_finite(m.uc) && rd_finite(m.vc) && m.rx > 0.0 && m.ry > 0.0 && rd_finite(m.rx) && rd_finite(m.ry);
            }
            mrec[(size_t)f * N + k] = m;
        }
    }
}

// A face's set-up relative to the pixel centre (ox, oy) (1/16-pixel units).  v0 .. v2: its vertices' records; a face of negative area
// is re-oriented by exchanging v1 and v2, so that e, q and the caller's records all speak of the same corners afterwards.
//   e[k]   the edge function opposite corner k at (ox, oy): positive inside, e[k] / area2 is corner k's barycentric weight
//   a[k], b[k]   its steps per PIXEL in x and y
//   q[k]   1 / (z_k area2)
// false: the face is not drawn (a vertex not ok, a vertex named twice, no area).
struct RdFace { long long e[3]; int a[3], b[3]; double q[3]; };
__device__ __forceinline__ void rd_edge(const RenderVertex& pa, const RenderVertex& pb, const RenderVertex& pk, int ox, int oy, long long area2,
                                        int k, RdFace* s) {
#pragma clang fp contract(off)
    const int dx = pb.sx - pa.sx, dy = pb.sy - pa.sy;
    s->e[k] = (long long)dx * (oy - pa.sy) - (long long)dy * (ox - pa.sx);
    s->a[k] = -16 * dy; s->b[k] = 16 * dx;
    s->q[k] = 1.0 / pk.z / (double)area2;
}
__device__ __forceinline__ bool rd_face_setup(unsigned ia, unsigned ib, unsigned ic, RenderVertex& v0, RenderVertex& v1, RenderVertex& v2,
                                              int ox, int oy, RdFace* s) {
    if (ia == ib || ib == ic || ia == ic) return false;
    if (!(v0.ok && v1.ok && v2.ok)) return false;
    long long area2 = (long long)(v1.sx - v0.sx) * (v2.sy - v0.sy) - (long long)(v1.sy - v0.sy) * (v2.sx - v0.sx);
    if (area2 == 0) return false;
    if (area2 < 0) { const RenderVertex t = v1; v1 = v2; v2 = t; area2 = -area2; }
    rd_edge(v1, v2, v0, ox, oy, area2, 0, s);
    rd_edge(v2, v0, v1, ox, oy, area2, 1, s);
    rd_edge(v0, v1, v2, ox, oy, area2, 2, s);
    return true;
}
// the fill rule's bias of an edge with steps (a, b): 0 on a top or left edge (E == 0 is inside), -1 elsewhere
__device__ __forceinline__ int rd_bias(int a, int b) { return (a > 0 || (a == 0 && b > 0)) ? 0 : -1; }

// the lane's share of a marker: d^2 = (du / rx)^2 + (dv / ry)^2 at the pixel centre (i + 0.5, j + 0.5)
__device__ __forceinline__ double rd_disc(double uc, double vc, double rx, double ry, int i, int j) {
#pragma clang fp contract(off)
    const double tx = ((double)i + 0.5 - uc) / rx, ty = ((double)j + 0.5 - vc) / ry;
    return tx * tx + ty * ty;
}

__global__ __launch_bounds__(RD_THREADS) void k_render_tiles(RenderArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    long long* s_e = reinterpret_cast<long long*>(lds_raw);                       // [3][RD_CHUNK]  face: e[k] + bias; marker: uc, vc, rx
    double* s_q = reinterpret_cast<double*>(lds_raw + RD_CHUNK * 24);             // [3][RD_CHUNK]  face: q[k]; marker: ry
    int* s_ab = reinterpret_cast<int*>(lds_raw + RD_CHUNK * 48);                  // [6][RD_CHUNK]  face: a[k], b[k]; marker: the depth's bits
    int* s_id = reinterpret_cast<int*>(lds_raw + RD_CHUNK * 72);                  // [RD_CHUNK]
    int* s_cnt = reinterpret_cast<int*>(lds_raw + RD_CHUNK * 76);                 // [2]: chunk c counts in s_cnt[c & 1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int px = tid & (RD_TILE - 1), py = tid / RD_TILE;
    const int tx0 = blockIdx.x * RD_TILE, ty0 = blockIdx.y * RD_TILE;
    const int pi = tx0 + px, pj = ty0 + py;
    const size_t f = blockIdx.z;
    const int ox = 16 * tx0 + 8, oy = 16 * ty0 + 8, span = 16 * (RD_TILE - 1);   // the tile's pixel centres: ox .. ox + span
    const RenderVertex* rec = A.rec + f * A.V;
    const RenderMarker* mrec = A.mrec + f * A.N;
    const int nitems = A.NF + A.N;
    float best = __builtin_inff();
    int bid = -1;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    for (int base = 0, c = 0; base < nitems; base += RD_CHUNK, c ^= 1) {
        const int item = base + tid;
        bool keep = false;
        RdFace fs;
        RenderMarker mk;
        if (item < A.NF) {
            unsigned ia, ib, ic;
            sd_face_ids(A.tris, A.w16 != 0, (unsigned)item, &ia, &ib, &ic);
            RenderVertex v0 = rec[ia], v1 = rec[ib], v2 = rec[ic];
            const int x0 = min(min(v0.sx, v1.sx), v2.sx), x1 = max(max(v0.sx, v1.sx), v2.sx);
            const int y0 = min(min(v0.sy, v1.sy), v2.sy), y1 = max(max(v0.sy, v1.sy), v2.sy);
            keep = rd_face_setup(ia, ib, ic, v0, v1, v2, ox, oy, &fs) && x1 >= ox && x0 <= ox + span && y1 >= oy && y0 <= oy + span;
        } else if (item < nitems) {
            mk = mrec[item - A.NF];
            // (1e-6 pixel of slack: the bounds are rounded sums, the pixel test below is the rule)
            keep = mk.ok && mk.uc + mk.rx + 1e-6 >= (double)tx0 + 0.5 && mk.uc - mk.rx - 1e-6 <= (double)tx0 + (RD_TILE - 0.5) &&
                   mk.vc + mk.ry + 1e-6 >= (double)ty0 + 0.5 && mk.vc - mk.ry - 1e-6 <= (double)ty0 + (RD_TILE - 0.5);
        }
        const unsigned long long bal = __ballot(keep);
        int wbase = 0;
        if (lane == 0) wbase = atomicAdd(&s_cnt[c], __popcll(bal));
        wbase = __shfl(wbase, 0);
        if (keep) {
            const int slot = wbase + __popcll(bal & ((1ull << lane) - 1ull));
            s_id[slot] = item;
            if (item < A.NF) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    s_e[k * RD_CHUNK + slot] = fs.e[k] + rd_bias(fs.a[k], fs.b[k]);
                    s_q[k * RD_CHUNK + slot] = fs.q[k];
                    s_ab[k * RD_CHUNK + slot] = fs.a[k];
                    s_ab[(3 + k) * RD_CHUNK + slot] = fs.b[k];
                }
            } else {
                s_e[slot] = __builtin_bit_cast(long long, mk.uc);
                s_e[RD_CHUNK + slot] = __builtin_bit_cast(long long, mk.vc);
                s_e[2 * RD_CHUNK + slot] = __builtin_bit_cast(long long, mk.rx);
                s_q[slot] = mk.ry;
                s_ab[slot] = __builtin_bit_cast(int, mk.depth);
            }
        }
        if (tid == 0) s_cnt[c ^ 1] = 0;   // (the next chunk's counter: nobody touches it before the barrier after this chunk's run)
        __syncthreads();
        const int cnt = s_cnt[c];
        for (int s = 0; s < cnt; ++s) {
            const int id = s_id[s];
            float z;
            if (id < A.NF) {
                const int a0 = s_ab[s], a1 = s_ab[RD_CHUNK + s], a2 = s_ab[2 * RD_CHUNK + s];
                const int b0 = s_ab[3 * RD_CHUNK + s], b1 = s_ab[4 * RD_CHUNK + s], b2 = s_ab[5 * RD_CHUNK + s];
                const long long e0 = s_e[s] + (long long)a0 * px + (long long)b0 * py;
                const long long e1 = s_e[RD_CHUNK + s] + (long long)a1 * px + (long long)b1 * py;
                const long long e2 = s_e[2 * RD_CHUNK + s] + (long long)a2 * px + (long long)b2 * py;
                if ((e0 | e1 | e2) < 0) continue;
                const double den = (double)(e0 - rd_bias(a0, b0)) * s_q[s] + (double)(e1 - rd_bias(a1, b1)) * s_q[RD_CHUNK + s] +
                                   (double)(e2 - rd_bias(a2, b2)) * s_q[2 * RD_CHUNK + s];
                z = (float)(1.0 / den);
            } else {
                const double d2 = rd_disc(__builtin_bit_cast(double, s_e[s]), __builtin_bit_cast(double, s_e[RD_CHUNK + s]),
                                          __builtin_bit_cast(double, s_e[2 * RD_CHUNK + s]), s_q[s], pi, pj);
                if (!(d2 <= 1.0)) continue;
                z = __builtin_bit_cast(float, s_ab[s]);
            }
            if (z < best || (z == best && id < bid)) { best = z; bid = id; }
        }
        __syncthreads();
    }
    if (pi >= A.W || pj >= A.H) return;
    const size_t at = (f * A.H + pj) * A.W + pi;
    if (A.ids) A.ids[at] = bid;
    if (A.depth) A.depth[at] = best;
    if (!A.rgb) return;
    double inten = A.ambient;
    const unsigned char* col = A.bg;
    if (bid >= A.NF) {
        const RenderMarker mk = mrec[bid - A.NF];
        const double d2 = rd_disc(mk.uc, mk.vc, mk.rx, mk.ry, pi, pj);
        inten = A.ambient + (1.0 - A.ambient) * sqrt(fmax(0.0, 1.0 - d2));
        col = A.prgb + 3 * (size_t)(bid - A.NF);
    } else if (bid >= 0) {
        unsigned ia, ib, ic;
        sd_face_ids(A.tris, A.w16 != 0, (unsigned)bid, &ia, &ib, &ic);
        RenderVertex v0 = rec[ia], v1 = rec[ib], v2 = rec[ic];
        RdFace fs;
        rd_face_setup(ia, ib, ic, v0, v1, v2, 16 * pi + 8, 16 * pj + 8, &fs);
        const double b0 = (double)fs.e[0] * fs.q[0], b1 = (double)fs.e[1] * fs.q[1], b2 = (double)fs.e[2] * fs.q[2];   // a corner's weight over its depth
        double n[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) n[i] = b0 * (double)v0.n[i] + b1 * (double)v1.n[i] + b2 * (double)v2.n[i];
        const double l2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        if (l2 > 0.0 && rd_finite(l2)) inten = A.ambient + (1.0 - A.ambient) * fmax(0.0, -(n[2] / sqrt(l2)));
        col = A.body;
    }
    unsigned char* o = A.rgb + at * 3;
    if (bid < 0) { o[0] = col[0]; o[1] = col[1]; o[2] = col[2]; }
    else {
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = (unsigned char)floor(255.0 * ((double)col[i] / 255.0) * inten + 0.5);
    }
}

}  // namespace

static void free_ptr(void* p) { if (p) hipFree(p); }

extern "C" void moshii_lbs32_free(void* l32) {
    Lbs32Model* lm = (Lbs32Model*)l32;
    free_ptr(lm->v_shaped); free_ptr(lm->posedirs_t); free_ptr(lm->weights); free_ptr(lm->J);
    free_ptr(lm->Pfrag); free_ptr(lm->perm); free_ptr(lm->tables); free_ptr(lm->dbgbuf);
    free_ptr(lm->Atr); free_ptr(lm->featF); free_ptr(lm->hcompf); free_ptr(lm->hmeanf); free_ptr(lm->varflag); free_ptr(lm->jtab); free_ptr(lm->hcj);
    free_ptr(lm->PfragX); free_ptr(lm->JSf); free_ptr(lm->Sft);
    memset(lm, 0, sizeof(*lm));
}

// Partition of every 64-vertex tile into four groups of 16 so that a group's vertices depend on few joints (its joint list is what
// the export kernel's blend walks, four joints per round; the workgroup meets at a barrier per block, so the tile's LARGEST list
// counts first, then the sum).  Start: the tile's vertices sorted by (strongest, second strongest) joint, cut into 16s; then pair
// swaps between groups while they lower (max rounds, sum of rounds, sum of joints).  mask[v] = the joints of vertex v (K <= 64).
// Returns order[tile * 64 + slot] = vertex id (or -1: padding behind V).
static std::vector<int> group_tiles(int V, int K, const double* wh, int NVT) {
    std::vector<int> order((size_t)NVT * LX_TV, -1);
    std::vector<unsigned long long> mask((size_t)NVT * LX_TV, 0ull);
    std::vector<int> key((size_t)NVT * LX_TV, 0);
    for (int v = 0; v < V; ++v) {
        int j1 = 0, j2 = -1;
        double w1 = -1.0, w2 = -1.0;
        unsigned long long m = 0;
        for (int j = 0; j < K; ++j) {
            const double w = std::fabs(wh[(size_t)v * K + j]);
            if (wh[(size_t)v * K + j] != 0.0) m |= 1ull << j;
            if (w > w1) { w2 = w1; j2 = j1; w1 = w; j1 = j; }
            else if (w > w2) { w2 = w; j2 = j; }
        }
        if (j2 < 0 || w2 <= 0.0) j2 = j1;
        mask[v] = m;
        key[v] = j1 * 64 + j2;
    }
    auto pc = [](unsigned long long m) { return __builtin_popcountll(m); };
    for (int t = 0; t < NVT; ++t) {
        int ids[LX_TV];
        for (int s = 0; s < LX_TV; ++s) ids[s] = t * LX_TV + s;
        std::stable_sort(ids, ids + LX_TV, [&](int a, int b) {
            const bool pa = a >= V, pb = b >= V;     // padding last
            if (pa != pb) return pb;
            return key[a] < key[b];
        });
        unsigned long long gm[4];
        auto umask = [&](int g) { unsigned long long m = 0; for (int s = 0; s < 16; ++s) m |= mask[ids[g * 16 + s]]; return m; };
        auto cost = [&](const unsigned long long* ms) {
            long mx = 0, sr = 0, sj = 0;
            for (int g = 0; g < 4; ++g) { const long n = pc(ms[g]), r = std::max(1L, (n + LX_JR - 1) / LX_JR); mx = std::max(mx, r); sr += r; sj += n; }
            return mx * 1000000L + sr * 1000L + sj;
        };
        for (int g = 0; g < 4; ++g) gm[g] = umask(g);
        long cur = cost(gm);
        for (int sweep = 0; sweep < 4; ++sweep) {
            bool improved = false;
            for (int a = 0; a < 4; ++a)
                for (int b = a + 1; b < 4; ++b)
                    for (int ia = 0; ia < 16; ++ia)
                        for (int ib = 0; ib < 16; ++ib) {
                            std::swap(ids[a * 16 + ia], ids[b * 16 + ib]);
                            unsigned long long ms[4] = {gm[0], gm[1], gm[2], gm[3]};
                            ms[a] = umask(a); ms[b] = umask(b);
                            const long c = cost(ms);
                            if (c < cur) { cur = c; gm[a] = ms[a]; gm[b] = ms[b]; improved = true; }
                            else std::swap(ids[a * 16 + ia], ids[b * 16 + ib]);
                        }
            if (!improved) break;
        }
        for (int s = 0; s < LX_TV; ++s) order[(size_t)t * LX_TV + s] = ids[s] < V ? ids[s] : -1;
    }
    return order;
}

extern "C" int moshii_lbs32_prepare(moshii_model_t m) {
    int V, K;
    moshii_internal_model_dims(m, &V, &K);
    Lbs32Model* lm = (Lbs32Model*)moshii_internal_l32(m);
    const int Vp = (V + 63) & ~63;
    const int nfeat = 9 * (K - 1);
    DevArena tmp;   // the reductions' buffers
    // any failure frees the whole copy: the next call finds no v_shaped and builds it again, never over half of one
    auto bad = [&](const char* what) {
        moshii_lbs32_free(lm);
        return moshii_internal_fail(MOSHII_ERR_HIP, (std::string("moshii_lbs32_prepare: device allocation failed: ") + what).c_str());
    };
    if (!lm->v_shaped) {
        if (hipMalloc((void**)&lm->v_shaped, (size_t)V * 3 * sizeof(float)) != hipSuccess) return bad("v_shaped");
        if (hipMalloc((void**)&lm->posedirs_t, (size_t)std::max(nfeat, 1) * 3 * Vp * sizeof(float)) != hipSuccess) return bad("posedirs_t");
        if (hipMalloc((void**)&lm->weights, (size_t)K * Vp * sizeof(float)) != hipSuccess) return bad("weights");
        if (hipMalloc((void**)&lm->J, (size_t)K * 3 * sizeof(float)) != hipSuccess) return bad("J");
        lm->Vp = Vp;
        hipLaunchKernelGGL(k_cvt_posedirs, dim3(2048), dim3(256), 0, 0, V, Vp, nfeat, moshii_internal_posedirs(m), lm->posedirs_t);
        hipLaunchKernelGGL(k_cvt_weights, dim3(512), dim3(256), 0, 0, V, Vp, K, moshii_internal_weights(m), lm->weights);
        // ---- MFMA-path model copy
        lm->mfma_ok = 0;
        const int NVT = (V + LX_TV - 1) / LX_TV, NG = NVT * 4;
        const int KS = (nfeat + 31) / 32;
        lm->NVT = NVT; lm->KS = KS; lm->K = K;
        lm->KJ = (K + 3) & ~3;
        const double* wh = moshii_internal_weights_host(m);
        bool ok = nfeat > 0 && K <= 64;
        std::vector<int> order, gnr, gjid, gx;
        std::vector<float> gw;
        int NRM = 1;
        if (ok) {
            order = group_tiles(V, K, wh, NVT);
            std::vector<std::vector<int>> lists(NG);
            for (int g = 0; g < NG; ++g) {
                unsigned long long mk = 0;
                for (int s = 0; s < 16; ++s) {
                    const int v = order[(size_t)g * 16 + s];
                    if (v >= 0) for (int j = 0; j < K; ++j) if (wh[(size_t)v * K + j] != 0.0) mk |= 1ull << j;
                }
                for (int j = 0; j < K; ++j) if (mk >> j & 1) lists[g].push_back(j);
                NRM = std::max(NRM, ((int)lists[g].size() + LX_JR - 1) / LX_JR);
            }
            ok = NRM <= LX_NRMAX;
            if (ok) {
                gnr.assign(NG, 1); gjid.assign((size_t)NG * NRM * LX_JR, 0); gx.assign((size_t)NG * 16, 0);
                gw.assign((size_t)NG * NRM * 16 * LX_JR, 0.0f);
                for (int g = 0; g < NG; ++g) {
                    const int nj = (int)lists[g].size();
                    gnr[g] = std::max(1, (nj + LX_JR - 1) / LX_JR);
                    for (int i = 0; i < nj; ++i) gjid[(size_t)g * NRM * LX_JR + i] = lists[g][i] * LX_JBYTES;
                    for (int s = 0; s < 16; ++s) {
                        const int v = order[(size_t)g * 16 + s];
                        // padding keeps its own column of the tile (beyond the valid floats of a row: written to the exchange, never stored)
                        int col = v >= 0 ? v % LX_TV : -1;
                        if (col < 0) {   // the free columns of this tile, in slot order
                            const int tile = g / 4, nvalid = std::min(LX_TV, V - tile * LX_TV);
                            int npad_before = 0;
                            for (int s2 = 0; s2 < (g % 4) * 16 + s; ++s2) if (order[(size_t)tile * LX_TV + s2] < 0) ++npad_before;
                            col = nvalid + npad_before;
                        }
                        gx[(size_t)g * 16 + s] = col * 12;
                        if (v >= 0) for (int i = 0; i < nj; ++i)
                            gw[(((size_t)g * NRM + i / LX_JR) * 16 + s) * LX_JR + i % LX_JR] = (float)wh[(size_t)v * K + lists[g][i]];
                    }
                }
            }
        }
        lm->NRM = NRM;
        if (ok) {
            double* d_part = tmp.alloc<double>(256);
            if (!d_part) return bad("the reduction buffer");
            hipLaunchKernelGGL(k_absmax, dim3(256), dim3(256), 0, 0, (size_t)V * 3 * nfeat, moshii_internal_posedirs(m), d_part);
            double part[256];
            if (hipMemcpy(part, d_part, sizeof(part), hipMemcpyDeviceToHost) != hipSuccess) return bad("the reduction buffer (copy)");
            double amax = 0.0;
            for (double p : part) amax = std::max(amax, p);
            // power-of-two scale that lifts the largest corrective to ~2^13: small entries stay normal in f16
            double pscale = 1.0;
            if (amax > 0.0) pscale = std::ldexp(1.0, 13 - (int)std::ceil(std::log2(amax)));
            lm->pscale = (float)pscale;
            lm->inv_pscale = (float)(1.0 / pscale);
            if (hipMalloc((void**)&lm->Pfrag, (size_t)NG * 3 * KS * 64 * 8 * sizeof(_Float16)) != hipSuccess) return bad("Pfrag");
            if (hipMalloc((void**)&lm->perm, order.size() * sizeof(int)) != hipSuccess) return bad("perm");
            // one allocation for the per-group tables (16-byte aligned parts): rounds | joint lists | exchange columns | rest positions | weights
            auto al16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
            lm->tab_gnr = 0;
            lm->tab_gjid = (unsigned)al16(gnr.size() * sizeof(int));
            lm->tab_gx = lm->tab_gjid + (unsigned)al16(gjid.size() * sizeof(int));
            lm->tab_vshs = lm->tab_gx + (unsigned)al16(gx.size() * sizeof(int));
            lm->tab_gw = lm->tab_vshs + (unsigned)((size_t)NG * 16 * 4 * sizeof(float));
            lm->tab_vsc = lm->tab_gw + (unsigned)al16(gw.size() * sizeof(float));     // per call: rest + still correctives (k_lbs_still)
            const size_t tab_bytes = lm->tab_vsc + (size_t)NG * 16 * 4 * sizeof(float);
            if (hipMalloc((void**)&lm->tables, tab_bytes) != hipSuccess) return bad("tables");
            hipMemset(lm->tables, 0, tab_bytes);
            if (hipMalloc((void**)&lm->dbgbuf, 1024 * sizeof(long long)) != hipSuccess) return bad("dbgbuf");
            hipMemset(lm->dbgbuf, 0, 1024 * sizeof(long long));
            hipMemcpy(lm->perm, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice);
            hipMemcpy(lm->tables + lm->tab_gx, gx.data(), gx.size() * sizeof(int), hipMemcpyHostToDevice);
            hipMemcpy(lm->tables + lm->tab_gnr, gnr.data(), gnr.size() * sizeof(int), hipMemcpyHostToDevice);
            hipMemcpy(lm->tables + lm->tab_gjid, gjid.data(), gjid.size() * sizeof(int), hipMemcpyHostToDevice);
            hipMemcpy(lm->tables + lm->tab_gw, gw.data(), gw.size() * sizeof(float), hipMemcpyHostToDevice);
            hipLaunchKernelGGL(k_pack_pfrag, dim3(4096), dim3(256), 0, 0, nfeat, KS, NG, pscale, lm->perm, moshii_internal_posedirs(m), lm->Pfrag);
            lm->mfma_ok = 1;
        }
    }
    // ---- the free shape block (declared, changed or cleared since the last prepare: moshii_model_set_free_shape clears l32_valid)
    {
        if (hipDeviceSynchronize() != hipSuccess) return bad("(hipDeviceSynchronize)");
        free_ptr(lm->PfragX); free_ptr(lm->JSf); free_ptr(lm->Sft);
        lm->PfragX = nullptr; lm->JSf = nullptr; lm->Sft = nullptr; lm->nshape = 0; lm->KSX = 0; lm->sxscale = 1.0f;
        int NB = 0, start = 0, E = 0;
        const double* JS = nullptr;
        const double* sd = moshii_internal_shape_block(m, &NB, &start, &E, &JS);
        if (E > 0) {
            if (hipMalloc((void**)&lm->JSf, (size_t)K * E * 4 * sizeof(float)) != hipSuccess) return bad("JSf");
            if (hipMalloc((void**)&lm->Sft, (size_t)E * 3 * Vp * sizeof(float)) != hipSuccess) return bad("Sft");
            hipLaunchKernelGGL(k_cvt_js, dim3((K * E + 255) / 256), dim3(256), 0, 0, K * E, JS, lm->JSf);
            hipLaunchKernelGGL(k_cvt_shapedirs, dim3(1024), dim3(256), 0, 0, V, Vp, NB, start, E, sd, lm->Sft);
            lm->nshape = E;
            // (k_lbs_prep<true> keeps a frame's feature row in LDS: bodies whose pose and shape k-steps pass its size take the plain kernel)
            if (lm->mfma_ok && lm->KS + (3 * E + 31) / 32 <= LBS_PREP_KSMAX) {
                double* d_part = tmp.alloc<double>(256);
                if (!d_part) return bad("the reduction buffer");
                hipLaunchKernelGGL(k_absmax_block, dim3(256), dim3(256), 0, 0, (size_t)V * 3, NB, start, E, sd, d_part);
                double part[256];
                if (hipMemcpy(part, d_part, sizeof(part), hipMemcpyDeviceToHost) != hipSuccess) return bad("the reduction buffer (copy)");
                double dmax = 0.0;
                for (double p : part) dmax = std::max(dmax, p);
                // Operand scales.  The accumulators carry pscale x metres; the block's directions can be far larger than the pose
                // correctives pscale was chosen for, so they are DIVIDED by a power of two sxscale that puts the largest at 2^7 .. 2^8
                // and the coefficients multiplied by it: both halves of both operands' (hi, lo) pairs then stay f16 normals with bits
                // to spare for centimetre-scale directions and coefficients of order 1, and nothing overflows below |c| ~ 100.
                double sx = 1.0;
                if (dmax > 0.0) sx = std::ldexp(1.0, (int)std::ceil(std::log2(dmax * (double)lm->pscale)) - 8);
                lm->sxscale = (float)sx;
                lm->KSX = (3 * E + 31) / 32;
                const int NG = lm->NVT * 4, KST = lm->KSX + lm->KS;
                if (hipMalloc((void**)&lm->PfragX, (size_t)NG * 3 * KST * 64 * 8 * sizeof(_Float16)) != hipSuccess) return bad("PfragX");
                hipLaunchKernelGGL(k_pack_pfrag_shape, dim3(4096), dim3(256), 0, 0, NB, start, E, lm->KSX, lm->KS, NG, (double)lm->pscale / sx, lm->perm, sd, lm->Pfrag, lm->PfragX);
            }
        }
    }
    hipLaunchKernelGGL(k_cvt_vsh, dim3((V * 3 + 255) / 256), dim3(256), 0, 0, V * 3, moshii_internal_vsh(m), lm->v_shaped);
    hipLaunchKernelGGL(k_cvt_vsh, dim3(1), dim3(256), 0, 0, K * 3, moshii_internal_J(m), lm->J);
    lm->jtab_valid = 0;
    if (lm->mfma_ok)   // rest positions in group order, x pscale (the accumulators start there)
        hipLaunchKernelGGL(k_pack_vsh, dim3((lm->NVT * LX_TV + 255) / 256), dim3(256), 0, 0, lm->NVT * LX_TV, lm->pscale, lm->perm, moshii_internal_vsh(m), reinterpret_cast<float*>(lm->tables + lm->tab_vshs));
    if (hipDeviceSynchronize() != hipSuccess) return bad("(hipDeviceSynchronize)");
    moshii_internal_l32_set_valid(m, 1);
    return MOSHII_OK;
}

extern "C" int moshii_internal_lbs_debug_times(void* lbs32, long long* out512x2) {   // (development: MOSHII_LBS_STOP=32)
    Lbs32Model* lm = (Lbs32Model*)lbs32;
    if (!lm->dbgbuf) return -1;
    hipDeviceSynchronize();
    return hipMemcpy(out512x2, lm->dbgbuf, 512 * 2 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

extern "C" hipError_t moshii_launch_lbs_f32(hipStream_t stream, const ModelDev* md, int F, const float* pose,
                                            const float* trans, const float* shape, float* verts, void* lbs32) {
    Lbs32Model* lmp = (Lbs32Model*)lbs32;
    const bool force_v0 = getenv("MOSHII_LBS_PLAIN") != nullptr;   // the plain f32 kernel (tests compare the two)
    const bool sh = shape != nullptr && lmp->nshape > 0;           // per-frame coefficients of the free shape block
    if (!lmp->mfma_ok || force_v0 || (sh && !lmp->PfragX)) {
        const Lbs32Model lm = *lmp;
        const size_t lds = (size_t)(md->P + md->K * 33) * sizeof(float);
        hipLaunchKernelGGL(k_lbs_f32_v0, dim3((md->V + 255) / 256, F), dim3(256), lds, stream, *md, lm, pose, trans, sh ? shape : (const float*)nullptr, verts);
        return hipGetLastError();
    }
    const int KSU = sh ? lmp->KS + lmp->KSX : lmp->KS;             // k-steps of this call's feature rows
    // The export kernel addresses the per-call scratch through buffer resources (2^31 - 1 bytes, 32-bit offsets; a load beyond the range
    // returns zeros, silently): a call that would pass that is cut into sub-calls of whole frame tiles (SMPL-H: 860 000 frames a piece).
    {
        const long long per16 = (long long)lmp->KJ * LX_JBYTES, per128 = (long long)KSU * LX_CHUNK;
        long long fmax = std::min(((0x7fffffffLL - 4096) / per16) * 16, ((0x7fffffffLL - 4096) / per128) * LX_TF);
        if (const char* es = getenv("MOSHII_LBS_FMAX")) fmax = std::min(fmax, (long long)std::max(LX_TF, atoi(es)));   // (tests: a small limit)
        fmax = fmax / LX_TF * LX_TF;
        if ((long long)F > fmax) {
            for (long long f0 = 0; f0 < F; f0 += fmax) {
                const int n = (int)std::min<long long>(fmax, F - f0);
                hipError_t e = moshii_launch_lbs_f32(stream, md, n, pose + (size_t)f0 * md->NP, trans + (size_t)f0 * 3,
                                                     sh ? shape + (size_t)f0 * lmp->nshape : (const float*)nullptr, verts + (size_t)f0 * md->V * 3, lbs32);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        }
    }
    const int Fpad = (F + LX_TF - 1) / LX_TF * LX_TF;
    if (Fpad > lmp->Fcap) {   // per-call scratch grows to the largest F seen (not stream-ordered: sync first)
        hipStreamSynchronize(stream);
        free_ptr(lmp->Atr);
        lmp->Atr = nullptr; lmp->Fcap = 0;
        const size_t na = (size_t)(Fpad / 16) * lmp->KJ * LX_JBYTES;
        hipError_t e = hipMalloc((void**)&lmp->Atr, na);
        if (e != hipSuccess) return e;
        // frames beyond F and joints beyond K are never written again: they stay zero
        e = hipMemset(lmp->Atr, 0, na);
        if (e != hipSuccess) return e;
        lmp->Fcap = Fpad;
    }
    {   // the features likewise, by bytes: a row has KS k-steps, or KSX + KS in a call with shape coefficients
        const long long nf = (long long)(Fpad / LX_TF) * KSU * LX_CHUNK;
        if (nf > lmp->featcap) {
            hipStreamSynchronize(stream);
            free_ptr(lmp->featF);
            lmp->featF = nullptr; lmp->featcap = 0;
            hipError_t e = hipMalloc((void**)&lmp->featF, (size_t)nf);
            if (e != hipSuccess) return e;
            // (every call writes the whole rows of its frames; frames beyond F are computed and dropped: finite values, zero at first)
            e = hipMemset(lmp->featF, 0, (size_t)nf);
            if (e != hipSuccess) return e;
            lmp->featcap = nf;
        }
    }
    if (!lmp->hmeanf) {   // f32 copies of the hand-pose map (stream-ordered: ahead of the first k_lbs_prep that reads them)
        const int nh = std::max(md->nhand_full, 1), nc = std::max(md->hand_dof * md->nhand_full, 1);
        hipError_t e = hipMalloc((void**)&lmp->hmeanf, (size_t)nh * sizeof(float));
        if (e != hipSuccess) return e;
        e = hipMalloc((void**)&lmp->hcompf, (size_t)nc * sizeof(float));
        if (e != hipSuccess) return e;
        if (md->hand_dof > 0) {
            hipLaunchKernelGGL(k_cvt_vsh, dim3((nh + 255) / 256), dim3(256), 0, stream, md->nhand_full, (const double*)md->hands_mean, lmp->hmeanf);
            hipLaunchKernelGGL(k_cvt_vsh, dim3((nc + 255) / 256), dim3(256), 0, stream, md->hand_dof * md->nhand_full, (const double*)md->comps, lmp->hcompf);
        }
    }
    if (!lmp->varflag) {   // k_lbs_prep marks the joints that move in a call with the call's number: never reset, never equal to an older call's
        hipError_t e = hipMalloc((void**)&lmp->varflag, 64 * sizeof(int));
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(lmp->varflag, 0, 64 * sizeof(int), stream);
        if (e != hipSuccess) return e;
        lmp->epoch = 0;
    }
    lmp->epoch = lmp->epoch >= 0x7ffffff0 ? 1 : lmp->epoch + 1;
    if (!lmp->jtab) {
        hipError_t e = hipMalloc((void**)&lmp->jtab, 64 * 16 * sizeof(float));
        if (e != hipSuccess) return e;
        e = hipMalloc((void**)&lmp->hcj, 64 * 64 * sizeof(float));
        if (e != hipSuccess) return e;
        lmp->jtab_valid = 0;
    }
    if (!lmp->jtab_valid) {   // (the joints move with the betas: moshii_lbs32_prepare clears the mark)
        hipLaunchKernelGGL(k_pack_jtab, dim3(1), dim3(64), 0, stream, *md, lmp->J, lmp->hcompf, lmp->hmeanf, lmp->jtab, lmp->hcj);
        lmp->jtab_valid = 1;
    }
    const Lbs32Model lm = *lmp;
    int dbg = 0;
    if (const char* es = getenv("MOSHII_LBS_STOP")) dbg = atoi(es) & 127;   // (development: phase timing by truncation / clock stamps; incomplete output)
    const dim3 pgrid(LBS_PREP_WAVES == 16 ? (F + 15) / 16 : ((F + 127) / 128) * 32);
    long long* const pstamps = (dbg & 16) ? lm.dbgbuf + 8 * 24 : (long long*)nullptr;
    if (sh) {
        hipLaunchKernelGGL(k_lbs_prep<true>, pgrid, dim3(64 * LBS_PREP_WAVES), 0, stream, *md, lm.jtab, lm.hcj, lm.hcompf, F, KSU, lm.KJ, pose, trans, lm.Atr, lm.featF, lm.varflag, lm.epoch,
                           pstamps, lm.JSf, shape, lm.nshape, lm.KSX, lm.sxscale);
        hipLaunchKernelGGL(k_lbs_still<true>, dim3(lm.NVT * 4), dim3(64), 0, stream, lm, lm.varflag, lm.epoch, (dbg & 8) ? 1 : 0);
    } else {
        hipLaunchKernelGGL(k_lbs_prep<false>, pgrid, dim3(64 * LBS_PREP_WAVES), 0, stream, *md, lm.jtab, lm.hcj, lm.hcompf, F, lm.KS, lm.KJ, pose, trans, lm.Atr, lm.featF, lm.varflag, lm.epoch,
                           pstamps, (const float*)nullptr, (const float*)nullptr, 0, 0, 1.0f);
        hipLaunchKernelGGL(k_lbs_still<false>, dim3(lm.NVT * 4), dim3(64), 0, stream, lm, lm.varflag, lm.epoch, (dbg & 8) ? 1 : 0);
    }
    const int NVT = lm.NVT, NFT = Fpad / LX_TF;
    int ncu = 0, devid = 0;
    hipGetDevice(&devid);
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, devid);
    // two workgroups per CU (a workgroup takes half a CU's registers and LDS), 8 XCDs
    int nslots = std::max(1, std::min(2 * (ncu > 0 ? ncu : 256) / 8, ((NVT + 7) / 8) * NFT));
    if (const char* es = getenv("MOSHII_LBS_SLOTS")) nslots = std::max(1, std::min(nslots, atoi(es)));   // (development: fewer workgroups per XCD)
    hipError_t e = hipFuncSetAttribute(sh ? reinterpret_cast<const void*>(k_lbs_export<true>) : reinterpret_cast<const void*>(k_lbs_export<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LX_LDS_BYTES);
    if (e != hipSuccess) return e;
    if (sh) hipLaunchKernelGGL(k_lbs_export<true>, dim3(8 * nslots), dim3(256), LX_LDS_BYTES, stream, lm, md->V, F, NVT, NFT, verts, lm.varflag, lm.epoch, lm.dbgbuf, dbg);
    else hipLaunchKernelGGL(k_lbs_export<false>, dim3(8 * nslots), dim3(256), LX_LDS_BYTES, stream, lm, md->V, F, NVT, NFT, verts, lm.varflag, lm.epoch, lm.dbgbuf, dbg);
    return hipGetLastError();
}

// ---- vertex normals / virtual markers: launches (the handle, its face table and the checks live in moshii_api.hip) ----
// All addressing is 64-bit per frame (no buffer resources): any F runs in one call, the gather kernel walks frames beyond its grid.
// *which (may be null): the kernel taken, *lds_bytes / *threads its dynamic LDS and workgroup size (moshii_last_launch_info)
extern "C" hipError_t moshii_launch_vertex_normals(hipStream_t stream, int V, int F, int f64, const void* verts, void* normals,
                                                   const unsigned* rows, const unsigned* pairs, int w16, const char** which,
                                                   int* lds_bytes, int* threads) {
    const char* none = nullptr;
    int i0 = 0, i1 = 0;
    if (!which) which = &none;
    if (!lds_bytes) lds_bytes = &i0;
    if (!threads) threads = &i1;
    *which = ""; *lds_bytes = 0; *threads = 256;
    if (F <= 0 || V <= 0) return hipSuccess;
    const dim3 ggrid((V + 63) / 64, std::min(F, 1024));
    if (f64) {
        *which = "k_vn_gather<double>";
        if (w16) hipLaunchKernelGGL((k_vn_gather<double, true>), ggrid, dim3(256), 0, stream, V, F, (const double*)verts, (double*)normals, rows, pairs);
        else hipLaunchKernelGGL((k_vn_gather<double, false>), ggrid, dim3(256), 0, stream, V, F, (const double*)verts, (double*)normals, rows, pairs);
        return hipGetLastError();
    }
    const char* ek = getenv("MOSHII_VN_KERNEL");   // "gather": the L2 kernel for the f32 call too (tests, tools/lbs_bench.py --normals)
    const size_t frame = (size_t)V * 12;
    if ((ek && !strcmp(ek, "gather")) || frame + 16 > VN_LDS_MAX) {
        *which = "k_vn_gather<float>";
        if (w16) hipLaunchKernelGGL((k_vn_gather<float, true>), ggrid, dim3(256), 0, stream, V, F, (const float*)verts, (float*)normals, rows, pairs);
        else hipLaunchKernelGGL((k_vn_gather<float, false>), ggrid, dim3(256), 0, stream, V, F, (const float*)verts, (float*)normals, rows, pairs);
        return hipGetLastError();
    }
    int ncu = 0, devid = 0;
    hipGetDevice(&devid);
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, devid);
    if (ncu <= 0) ncu = 256;
    // frames a workgroup keeps resident: a big body one (a CU holds one workgroup), a small body as many as leave room for a second
    // workgroup on the CU, but no more than spread the call over every CU twice
    int G = 1;
    if (frame + 16 <= VN_LDS_PAIR) G = (int)std::max<size_t>(1, std::min<size_t>((VN_LDS_PAIR - 16) / frame, ((size_t)F + 2 * ncu - 1) / (2 * ncu)));
    const size_t lds = (((size_t)G * V * 3 + 3) * sizeof(float) + 15) & ~(size_t)15;
    const int per_cu = lds <= VN_LDS_PAIR ? 2 : 1;
    const int grid = (int)std::min<long long>(((long long)F + G - 1) / G, (long long)per_cu * ncu);
    *which = "k_vn_lds"; *lds_bytes = (int)lds; *threads = VN_THREADS;
    const void* kern = w16 ? reinterpret_cast<const void*>(k_vn_lds<true>) : reinterpret_cast<const void*>(k_vn_lds<false>);
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   // (the opt-in above 64 KB)
    if (e != hipSuccess) return e;
    if (w16) hipLaunchKernelGGL(k_vn_lds<true>, dim3(grid), dim3(VN_THREADS), lds, stream, V, F, G, (const float*)verts, (float*)normals, rows, pairs);
    else hipLaunchKernelGGL(k_vn_lds<false>, dim3(grid), dim3(VN_THREADS), lds, stream, V, F, G, (const float*)verts, (float*)normals, rows, pairs);
    return hipGetLastError();
}

// markers[nf][M][3] (and mnormals, or null) of the meshes verts[nf][V][3]; vids / dist on the device
extern "C" hipError_t moshii_launch_marker_normals(hipStream_t stream, int V, int nf, int M, int f64, const void* verts, const int* vids,
                                                   const double* dist, void* markers, void* mnormals, const unsigned* rows,
                                                   const unsigned* pairs, int w16) {
    if (nf <= 0 || M <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((long long)nf * M + 63) / 64));
    if (f64) {
        if (w16) hipLaunchKernelGGL((k_vn_markers<double, true>), grid, dim3(256), 0, stream, V, nf, M, (const double*)verts, vids, dist, (double*)markers, (double*)mnormals, rows, pairs);
        else hipLaunchKernelGGL((k_vn_markers<double, false>), grid, dim3(256), 0, stream, V, nf, M, (const double*)verts, vids, dist, (double*)markers, (double*)mnormals, rows, pairs);
    } else {
        if (w16) hipLaunchKernelGGL((k_vn_markers<float, true>), grid, dim3(256), 0, stream, V, nf, M, (const float*)verts, vids, dist, (float*)markers, (float*)mnormals, rows, pairs);
        else hipLaunchKernelGGL((k_vn_markers<float, false>), grid, dim3(256), 0, stream, V, nf, M, (const float*)verts, vids, dist, (float*)markers, (float*)mnormals, rows, pairs);
    }
    return hipGetLastError();
}

// ---- signed point-to-mesh distance: launches (the handle, its tables and the checks live in moshii_api.hip) ----
// face[F x N] receives the search's winners and then the face ids: never null here.  tris: the handle's face table (four 16-bit
// fields a face while w16, else three 32-bit ids).  *which: the search kernel taken.
template <class T, int PB>
static hipError_t sd_launch_gather(hipStream_t stream, int V, int NF, long long F, int N, const T* verts, const T* points,
                                   const unsigned* tris, int w16, int* face) {
    const long long items = F * ((N + PB - 1) / PB);
    const dim3 grid((unsigned)std::min<long long>((items + 3) / 4, 1 << 20));
    if (w16) hipLaunchKernelGGL((k_sd_gather<T, PB, true>), grid, dim3(256), 0, stream, V, NF, F, N, verts, points, tris, face);
    else hipLaunchKernelGGL((k_sd_gather<T, PB, false>), grid, dim3(256), 0, stream, V, NF, F, N, verts, points, tris, face);
    return hipGetLastError();
}
template <int PB>
static hipError_t sd_launch_lds(hipStream_t stream, int V, int NF, int F, int G, int N, int grid, size_t lds, const float* verts,
                                const float* points, const unsigned* tris, int w16, int* face) {
    const void* kern = w16 ? reinterpret_cast<const void*>(k_sd_lds<PB, true>) : reinterpret_cast<const void*>(k_sd_lds<PB, false>);
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   // (the opt-in above 64 KB)
    if (e != hipSuccess) return e;
    if (w16) hipLaunchKernelGGL((k_sd_lds<PB, true>), dim3(grid), dim3(SD_THREADS), lds, stream, V, NF, F, G, N, verts, points, tris, face);
    else hipLaunchKernelGGL((k_sd_lds<PB, false>), dim3(grid), dim3(SD_THREADS), lds, stream, V, NF, F, G, N, verts, points, tris, face);
    return hipGetLastError();
}
template <class T>
static hipError_t sd_launch_finish(hipStream_t stream, int V, long long total, int N, const T* verts, const T* points, const unsigned* tris,
                                   int w16, const unsigned* rows, const unsigned* pairs, T* dist, int* face, int* part, T* nearest) {
    const dim3 grid((unsigned)std::min<long long>((total + 63) / 64, 1 << 20));
    if (w16) hipLaunchKernelGGL((k_sd_finish<T, true>), grid, dim3(256), 0, stream, V, total, N, verts, points, tris, rows, pairs, dist, face, part, nearest);
    else hipLaunchKernelGGL((k_sd_finish<T, false>), grid, dim3(256), 0, stream, V, total, N, verts, points, tris, rows, pairs, dist, face, part, nearest);
    return hipGetLastError();
}

extern "C" hipError_t moshii_launch_surface_distance(hipStream_t stream, int V, int NF, int F, int N, int f64, const void* verts,
                                                     const void* points, const unsigned* tris, int w16, const unsigned* rows,
                                                     const unsigned* pairs, void* dist, int* face, int* part, void* nearest,
                                                     const char** which, int* lds_bytes, int* threads) {
    const char* none = nullptr;
    int i0 = 0, i1 = 0;
    if (!which) which = &none;
    if (!lds_bytes) lds_bytes = &i0;
    if (!threads) threads = &i1;
    *which = ""; *lds_bytes = 0; *threads = 256;
    if (F <= 0 || N <= 0 || V <= 0) return hipSuccess;
    const long long total = (long long)F * N;
    // points a wave takes together (a triangle is loaded once for all of them): four where that still leaves a workgroup's waves busy
    const bool pb4 = N > 16;
    hipError_t e;
    if (f64) {
        *which = "k_sd_gather<double>";
        e = pb4 ? sd_launch_gather<double, 4>(stream, V, NF, F, N, (const double*)verts, (const double*)points, tris, w16, face)
                : sd_launch_gather<double, 1>(stream, V, NF, F, N, (const double*)verts, (const double*)points, tris, w16, face);
        if (e != hipSuccess) return e;
        return sd_launch_finish<double>(stream, V, total, N, (const double*)verts, (const double*)points, tris, w16, rows, pairs, (double*)dist, face, part, (double*)nearest);
    }
    // The L2 kernel is the default for f32 too: measured on 4000 SMPL-H frames x 53 points it takes 7.4 ms where the staged kernel takes
    // 11.6 (profiles/surface_distance.txt).  MOSHII_SD_KERNEL=lds asks for the staged kernel where a frame fits
    // (tests, tools/lbs_bench.py --surface-distance); same bits either way.
    const char* ek = getenv("MOSHII_SD_KERNEL");
    const size_t frame = (size_t)V * 12;
    if (!(ek && !strcmp(ek, "lds")) || frame + 16 > VN_LDS_MAX) {
        *which = "k_sd_gather<float>";
        e = pb4 ? sd_launch_gather<float, 4>(stream, V, NF, F, N, (const float*)verts, (const float*)points, tris, w16, face)
                : sd_launch_gather<float, 1>(stream, V, NF, F, N, (const float*)verts, (const float*)points, tris, w16, face);
    } else {
        int ncu = 0, devid = 0;
        hipGetDevice(&devid);
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, devid);
        if (ncu <= 0) ncu = 256;
        // frames a workgroup keeps resident, as the normals kernel sizes them: a big body one, a small body as many as leave room for a
        // second workgroup on the CU, but no more than spread the call over every CU twice
        int G = 1;
        if (frame + 16 <= VN_LDS_PAIR) G = (int)std::max<size_t>(1, std::min<size_t>((VN_LDS_PAIR - 16) / frame, ((size_t)F + 2 * ncu - 1) / (2 * ncu)));
        const size_t lds = (((size_t)G * V * 3 + 3) * sizeof(float) + 15) & ~(size_t)15;
        const int per_cu = lds <= VN_LDS_PAIR ? 2 : 1;
        const int grid = (int)std::min<long long>(((long long)F + G - 1) / G, (long long)per_cu * ncu);
        *which = "k_sd_lds"; *lds_bytes = (int)lds; *threads = SD_THREADS;
        e = pb4 ? sd_launch_lds<4>(stream, V, NF, F, G, N, grid, lds, (const float*)verts, (const float*)points, tris, w16, face)
                : sd_launch_lds<1>(stream, V, NF, F, G, N, grid, lds, (const float*)verts, (const float*)points, tris, w16, face);
    }
    if (e != hipSuccess) return e;
    return sd_launch_finish<float>(stream, V, total, N, (const float*)verts, (const float*)points, tris, w16, rows, pairs, (float*)dist, face, part, (float*)nearest);
}

// ---- posed joints / world joint rotations: launch (the checks live in moshii_api.hip) ----
// One wave per frame, JT_WAVES frames a workgroup; needs nothing on the handle beyond the model arrays in *md.  rot may be null.
// *which: the kernel's name for moshii_last_launch_info, *threads its workgroup size.
template <class T>
static hipError_t joints_launch(hipStream_t stream, const ModelDev& md, int F, const T* pose, const T* trans, const T* shape, T* joints, T* rot) {
    const dim3 grid((unsigned)(((long long)F + JT_WAVES - 1) / JT_WAVES));
    if (shape) hipLaunchKernelGGL((k_joints<T, true>), grid, dim3(64 * JT_WAVES), 0, stream, md, F, pose, trans, shape, joints, rot);
    else hipLaunchKernelGGL((k_joints<T, false>), grid, dim3(64 * JT_WAVES), 0, stream, md, F, pose, trans, shape, joints, rot);
    return hipGetLastError();
}

extern "C" hipError_t moshii_launch_joints(hipStream_t stream, const ModelDev* md, int F, int f64, const void* pose, const void* trans,
                                           const void* shape, void* joints, void* rot, const char** which, int* threads) {
    if (which) *which = "";
    if (threads) *threads = 64 * JT_WAVES;
    if (F <= 0) return hipSuccess;
    if (which) *which = f64 ? (shape ? "k_joints_shape<double>" : "k_joints<double>") : (shape ? "k_joints_shape<float>" : "k_joints<float>");
    if (f64) return joints_launch<double>(stream, *md, F, (const double*)pose, (const double*)trans, (const double*)shape, (double*)joints, (double*)rot);
    return joints_launch<float>(stream, *md, F, (const float*)pose, (const float*)trans, (const float*)shape, (float*)joints, (float*)rot);
}

// ---- shaded previews: launches (the handle, the scratch layout and the checks live in moshii_api.hip) ----
// nf frames (at most 65 535: grid.z): project the vertices and markers of every frame, then one workgroup a tile and frame.  args->rec /
// args->mrec receive the records; cams on the device, cam_stride 0 (one camera for all frames) or 1; points / radius null when N == 0.
// *which, *lds_bytes, *threads: k_render_tiles for moshii_last_launch_info.
extern "C" hipError_t moshii_launch_render(hipStream_t stream, int nf, int f64, const void* verts, const void* normals, const void* points,
                                           const double* radius, const moshii_camera* cams, int cam_stride, const RenderArgs* args,
                                           const char** which, int* lds_bytes, int* threads) {
    if (which) *which = "";
    if (lds_bytes) *lds_bytes = 0;
    if (threads) *threads = RD_THREADS;
    if (nf <= 0) return hipSuccess;
    const RenderArgs& A = *args;
    const dim3 pgrid((unsigned)((A.V + A.N + 255) / 256), (unsigned)std::min(nf, 1024));
    RenderVertex* rec = const_cast<RenderVertex*>(A.rec);
    RenderMarker* mrec = const_cast<RenderMarker*>(A.mrec);
    if (f64) hipLaunchKernelGGL(k_render_project<double>, pgrid, dim3(256), 0, stream, A.V, A.N, nf, cam_stride, cams, (const double*)verts, (const double*)normals, (const double*)points, radius, rec, mrec);
    else hipLaunchKernelGGL(k_render_project<float>, pgrid, dim3(256), 0, stream, A.V, A.N, nf, cam_stride, cams, (const float*)verts, (const float*)normals, (const float*)points, radius, rec, mrec);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_render_tiles), hipFuncAttributeMaxDynamicSharedMemorySize, RD_LDS_BYTES);   // (the opt-in above 64 KB)
    if (e != hipSuccess) return e;
    if (which) *which = "k_render_tiles";
    if (lds_bytes) *lds_bytes = RD_LDS_BYTES;
    const dim3 tgrid((unsigned)((A.W + RD_TILE - 1) / RD_TILE), (unsigned)((A.H + RD_TILE - 1) / RD_TILE), (unsigned)nf);
    hipLaunchKernelGGL(k_render_tiles, tgrid, dim3(RD_THREADS), RD_LDS_BYTES, stream, A);
    return hipGetLastError();
}

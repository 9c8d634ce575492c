// libmoshii C ABI (include/moshii.h): handles, setup kernels, host-side staging and launch logic.
#include "../../include/moshii.h"
#include "moshii_dev.h"
#include "dev_mem.h"
#include "export_plan.h"
#include "solve_plan.h"
#include "stagei_views.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

extern "C" hipError_t moshii_launch_chain_solve(int nblk, int xt, int n_chains, size_t lds_bytes, hipStream_t stream,
                                                const ChainDev* chains, const ModelDev* md, const PriorDev* pr,
                                                const OptsDev* op, const ChainLayout* ly, int coop_g);
extern "C" hipError_t moshii_launch_markers(int F, size_t lds_bytes, hipStream_t stream, const AttachDev* att,
                                            const ModelDev* md, const ChainLayout* ly, const double* pose,
                                            const double* trans, double* out);
extern "C" hipError_t moshii_launch_lbs_f32(hipStream_t stream, const ModelDev* md, int F, const float* pose,
                                            const float* trans, const float* shape, float* verts, void* lbs32);
extern "C" hipError_t moshii_launch_vertex_normals(hipStream_t stream, int V, int F, int f64, const void* verts, void* normals,
                                                   const unsigned* rows, const unsigned* pairs, int w16, const char** which,
                                                   int* lds_bytes, int* threads);
extern "C" hipError_t moshii_launch_marker_normals(hipStream_t stream, int V, int nf, int M, int f64, const void* verts, const int* vids,
                                                   const double* dist, void* markers, void* mnormals, const unsigned* rows,
                                                   const unsigned* pairs, int w16);
extern "C" hipError_t moshii_launch_surface_distance(hipStream_t stream, int V, int NF, int F, int N, int f64, const void* verts,
                                                     const void* points, const unsigned* tris, int w16, const unsigned* rows,
                                                     const unsigned* pairs, void* dist, int* face, int* part, void* nearest,
                                                     const char** which, int* lds_bytes, int* threads);
extern "C" hipError_t moshii_launch_joints(hipStream_t stream, const ModelDev* md, int F, int f64, const void* pose, const void* trans,
                                           const void* shape, void* joints, void* rot, const char** which, int* threads);
extern "C" hipError_t moshii_launch_render(hipStream_t stream, int nf, int f64, const void* verts, const void* normals, const void* points,
                                           const double* radius, const moshii_camera* cams, int cam_stride, const RenderArgs* args,
                                           const char** which, int* lds_bytes, int* threads);

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(MOSHII_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

// a failed device allocation or copy of `what` (an arena or a staging helper)
template <class Mem>
int fail_mem(const Mem& mem, const std::string& what) {
    return fail(MOSHII_ERR_HIP, what + ": device allocation or copy failed: " + hipGetErrorString(mem.err()));
}

}  // namespace

extern "C" int moshii_internal_fail(int code, const char* msg) { return fail(code, msg); }   // (dev_mem.h, lbs_forward.hip)
extern "C" void moshii_lbs32_free(void* l32);                                                // lbs_forward.hip

struct moshii_model_s {
    int V = 0, K = 0, NB = 0, P = 0, NP = 0, body_dof = 0, hand_dof = 0, nhand_full = 0, maxdepth = 0;
    std::vector<int> parents, depth;
    std::vector<double> weights_host;   // [V][K] (attachment packing)
    DevArena mem;                       // what moshii_model_create makes; the d_* below are views for dev() and the kernels
    DevArena shape_mem;                 // d_JS, replaced as a whole by moshii_model_set_free_shape
    DevArena face_mem;                  // d_vn_rows, d_vn_pairs, d_sd_tris, replaced as a whole by moshii_model_set_faces
    double *d_vt = nullptr, *d_shapedirs = nullptr, *d_posedirs = nullptr, *d_weights = nullptr, *d_Jreg = nullptr;
    double *d_vsh = nullptr, *d_J = nullptr, *d_hands_mean = nullptr, *d_comps = nullptr;
    double* d_JS = nullptr;             // [K][nshape][3] (moshii_model_set_free_shape)
    int shape_start = 0, nshape = 0;
    Scratch qscratch;                   // per-chain shape-derivative scratch of the extended chain kernel
    Scratch coopbuf;                    // exchange slots + flags of cooperative chains (moshii_dev.h: CoopDev)
    Scratch handoff;                    // entry / final states and hand-off deviations of a chunked solve's chunks
    int *d_parents = nullptr, *d_depth = nullptr, *d_comp_lo = nullptr, *d_comp_hi = nullptr, *d_col_lo = nullptr, *d_col_hi = nullptr;
    unsigned long long* d_anc = nullptr;
    bool betas_set = false;
    Lbs32Model l32 = {};                // the f32 export's copy of the model (lbs_forward.hip builds, grows and frees it)
    bool l32_valid = false;
    ~moshii_model_s() { moshii_lbs32_free(&l32); }
    Scratch scratch;
    // moshii_model_set_faces: vertex -> incident-corner table (CSR; lbs_forward.hip, "vertex normals"); null = no faces
    unsigned *d_vn_rows = nullptr, *d_vn_pairs = nullptr;
    int vn_w16 = 0;
    Scratch vmscratch;                  // moshii_virtual_markers_*: a batch of full meshes + the marker ids and distances
    // the triangles themselves for moshii_surface_distance_* (four 16-bit fields a face while vn_w16, else three 32-bit ids)
    unsigned* d_sd_tris = nullptr;
    int n_faces = 0;
    Scratch sdscratch;                  // moshii_surface_distance_* without a `face` output: the search's winners
    ModelDev dev() const {
        ModelDev md;
        md.V = V; md.K = K; md.P = P; md.NP = NP; md.body_dof = body_dof; md.hand_dof = hand_dof;
        md.nhand_full = nhand_full; md.maxdepth = maxdepth;
        md.parents = as_gp(d_parents); md.J = as_gp(d_J); md.hands_mean = as_gp(d_hands_mean); md.comps = as_gp(d_comps);
        md.comp_lo = as_gp(d_comp_lo); md.comp_hi = as_gp(d_comp_hi); md.col_lo = as_gp(d_col_lo); md.col_hi = as_gp(d_col_hi);
        md.anc = as_gp(d_anc); md.depth = as_gp(d_depth);
        md.nshape = nshape; md.JS = as_gp(d_JS);
        return md;
    }
};

struct moshii_prior_s {
    int G = 0, npose = 0;
    DevArena mem;
    double *d_means = nullptr, *d_chols = nullptr, *d_halfprec = nullptr, *d_neglogw = nullptr, *d_cnorm = nullptr;
    PriorDev dev() const {
        PriorDev p; p.G = G; p.npose = npose; p.means = as_gp(d_means); p.chols = as_gp(d_chols); p.halfprec = as_gp(d_halfprec);
        p.neglogw = as_gp(d_neglogw); p.cnorm = as_gp(d_cnorm);
        return p;
    }
};

struct moshii_attach_s {
    moshii_model_t model = nullptr;
    int M = 0, Nv = 0, Nvp = 0, NW = 0;
    DevArena mem;
    double *d_vsh = nullptr, *d_Pt = nullptr, *d_Pj = nullptr, *d_ww = nullptr, *d_coef = nullptr, *d_Ssh = nullptr;
    int nshape = 0;                     // free shape block gathered at creation (0: none)
    int* d_wj = nullptr;
    int* d_vids = nullptr;
    AttachDev* d_self = nullptr;
    AttachDev host_view;
};

namespace {

// ---- setup kernels --------------------------------------------------------------------------
__global__ void k_vshaped(int V, int NB, int nb, const double* __restrict__ vt, const double* __restrict__ sd,
                          const double* __restrict__ betas, double* __restrict__ vsh) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // (v, i)
    if (idx >= V * 3) return;
    const double* row = sd + (size_t)idx * NB;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += row[b] * betas[b];
    vsh[idx] = vt[idx] + s;
}

__global__ void k_joints(int V, const double* __restrict__ Jreg, const double* __restrict__ vsh, double* __restrict__ J) {
    const int k = blockIdx.x;
    __shared__ double red[3][256];
    double s[3] = {0.0, 0.0, 0.0};
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        const double w = Jreg[(size_t)k * V + v];
        if (w != 0.0) { s[0] += w * vsh[v * 3 + 0]; s[1] += w * vsh[v * 3 + 1]; s[2] += w * vsh[v * 3 + 2]; }
    }
    for (int i = 0; i < 3; ++i) red[i][threadIdx.x] = s[i];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) for (int i = 0; i < 3; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 3) J[k * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void k_pack_attach(int Nv, int Nvp, int K, const int* __restrict__ vids, const double* __restrict__ posedirs,
                              const double* __restrict__ vsh, double* __restrict__ Pt, double* __restrict__ Pj,
                              double* __restrict__ vsh_out) {
    const int nfeat = 9 * (K - 1);
    const size_t total = (size_t)(K - 1) * 27 * Nvp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int a = (int)(idx % Nvp);
        const int r = (int)(idx / Nvp);           // (k-1)*27 + i*9 + e
        const int km1 = r / 27, q = r % 27;
        double v = 0.0;
        if (a < Nv) v = posedirs[((size_t)vids[a] * 3 + q / 9) * nfeat + 9 * km1 + q % 9];
        Pt[idx] = v;
        if (a < Nv) {   // Pj[k-1][s][q/2][m] as 16-byte pairs, marker index fastest (a = 3 m + s): see AttachDev
            const int M = Nv / 3, mk = a / 3, sv = a % 3;
            Pj[((((size_t)km1 * 3 + sv) * 14 + q / 2) * M + mk) * 2 + (q & 1)] = v;
            if (q == 26) Pj[((((size_t)km1 * 3 + sv) * 14 + 13) * M + mk) * 2 + 1] = 0.0;
        }
    }
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < Nv * 3) vsh_out[t] = vsh[(size_t)vids[t / 3] * 3 + t % 3];
}

// JS[k][e][i] = sum_v Jreg[k][v] shapedirs[v][i][start + e]: the regressed joints' derivative wrt the free shape block.
__global__ void k_shape_joints(int V, int NB, int start, int E, const double* __restrict__ Jreg, const double* __restrict__ sd,
                               double* __restrict__ JS) {
    const int k = blockIdx.x / E, e = blockIdx.x % E;
    __shared__ double red[3][256];
    double s[3] = {0.0, 0.0, 0.0};
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        const double w = Jreg[(size_t)k * V + v];
        if (w != 0.0)
            for (int i = 0; i < 3; ++i) s[i] += w * sd[((size_t)v * 3 + i) * NB + start + e];
    }
    for (int i = 0; i < 3; ++i) red[i][threadIdx.x] = s[i];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) for (int i = 0; i < 3; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 3) JS[((size_t)k * E + e) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// Ssh[e][i][a] = shapedirs[vids[a]][i][start + e]  (vertex index fastest; zero in the padding)
__global__ void k_pack_shape(int Nv, int Nvp, int NB, int start, int E, const int* __restrict__ vids,
                             const double* __restrict__ sd, double* __restrict__ Ssh) {
    const size_t total = (size_t)E * 3 * Nvp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int a = (int)(idx % Nvp);
        const int r = (int)(idx / Nvp);   // e*3 + i
        Ssh[idx] = (a < Nv) ? sd[((size_t)vids[a] * 3 + r % 3) * NB + start + r / 3] : 0.0;
    }
}

// Reference-precision full-mesh LBS: one block = 256 vertices of one frame.
// SH: a row of free-shape coefficients per frame (moshii_lbs_forward_shape_f64): the rest positions gain the block's columns of
// shapedirs, the joints JS . shape[f] (LDS copy sJ); without it the frozen rest positions and joints, as before.
template <bool SH>
__global__ void k_lbs_f64(ModelDev md, const double* __restrict__ vsh, const double* __restrict__ posedirs,
                          const double* __restrict__ weights, const double* __restrict__ pose,
                          const double* __restrict__ trans, double* __restrict__ out,
                          const double* __restrict__ shapedirs, int NB, int sstart, const double* __restrict__ shape) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int K = md.K, P = md.P;
    double* fullpose = sm;            // P
    double* Rl = fullpose + P;        // K*9
    double* Rw = Rl + K * 9;          // K*9
    double* tw = Rw + K * 9;          // K*3
    double* feat = tw + K * 3;        // K*9
    double* sJ = feat + K * 9;        // K*3 (SH only): this frame's joints
    const int f = blockIdx.y, tid = threadIdx.x;
    const int E = SH ? md.nshape : 0;
    const double* cf = SH ? shape + (size_t)f * E : nullptr;
    if (SH) {
        for (int d = tid; d < K * 3; d += blockDim.x) {
            double s = md.J[d];
            for (int e = 0; e < E; ++e) s += md.JS[((size_t)(d / 3) * E + e) * 3 + d % 3] * cf[e];
            sJ[d] = s;
        }
    }
    auto Jat = [&](int d) -> double { if (SH) return sJ[d]; return md.J[d]; };
    const double* ps = pose + (size_t)f * md.NP;
    for (int d = tid; d < P; d += blockDim.x) {
        double v;
        if (d < md.body_dof) v = ps[d];
        else {
            const int h = d - md.body_dof;
            v = md.hands_mean[h];
            for (int i = 0; i < md.hand_dof; ++i) v += ps[md.body_dof + i] * md.comps[i * md.nhand_full + h];
        }
        fullpose[d] = v;
    }
    __syncthreads();
    if (tid < K) {
        const double x = fullpose[3 * tid], y = fullpose[3 * tid + 1], z = fullpose[3 * tid + 2];
        const double t2 = x * x + y * y + z * z;
        double a, b;
        if (t2 < 1e-6) { a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0; b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0; }
        else { const double t = sqrt(t2); a = sin(t) / t; b = (1.0 - cos(t)) / t2; }
        const double K2[9] = {x * x - t2, x * y, x * z, x * y, y * y - t2, y * z, x * z, y * z, z * z - t2};
        const double Km[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
        for (int e = 0; e < 9; ++e) {
            const double id = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
            const double r = id + a * Km[e] + b * K2[e];
            Rl[tid * 9 + e] = r;
            feat[tid * 9 + e] = r - id;
        }
    }
    __syncthreads();
    if (tid == 0) {   // serial chain: K <= 64 joints
        for (int e = 0; e < 9; ++e) Rw[e] = Rl[e];
        for (int i = 0; i < 3; ++i) tw[i] = Jat(i);
        for (int k = 1; k < K; ++k) {
            const int p = md.parents[k];
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j)
                    Rw[k * 9 + i * 3 + j] = Rw[p * 9 + i * 3 + 0] * Rl[k * 9 + 0 * 3 + j] + Rw[p * 9 + i * 3 + 1] * Rl[k * 9 + 1 * 3 + j] +
                                            Rw[p * 9 + i * 3 + 2] * Rl[k * 9 + 2 * 3 + j];
                tw[k * 3 + i] = Rw[p * 9 + i * 3 + 0] * (Jat(k * 3 + 0) - Jat(p * 3 + 0)) + Rw[p * 9 + i * 3 + 1] * (Jat(k * 3 + 1) - Jat(p * 3 + 1)) +
                                Rw[p * 9 + i * 3 + 2] * (Jat(k * 3 + 2) - Jat(p * 3 + 2)) + tw[p * 3 + i];
            }
        }
    }
    __syncthreads();
    const int v = blockIdx.x * blockDim.x + tid;
    if (v >= md.V) return;
    const int nfeat = 9 * (K - 1);
    double vp[3];
    for (int i = 0; i < 3; ++i) {
        const double* row = posedirs + ((size_t)v * 3 + i) * nfeat;
        double s = 0.0;
        for (int q = 0; q < nfeat; ++q) s += row[q] * feat[9 + q];
        if (SH) {
            const double* srow = shapedirs + ((size_t)v * 3 + i) * NB + sstart;
            for (int e = 0; e < E; ++e) s += srow[e] * cf[e];
        }
        vp[i] = vsh[v * 3 + i] + s;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < K; ++j) {
        const double w = weights[(size_t)v * K + j];
        if (w == 0.0) continue;
        const double dx = vp[0] - Jat(j * 3 + 0), dy = vp[1] - Jat(j * 3 + 1), dz = vp[2] - Jat(j * 3 + 2);
        for (int i = 0; i < 3; ++i)
            acc[i] += w * (Rw[j * 9 + i * 3 + 0] * dx + Rw[j * 9 + i * 3 + 1] * dy + Rw[j * 9 + i * 3 + 2] * dz + tw[j * 3 + i]);
    }
    const double* tr = trans + (size_t)f * 3;
    double* o = out + ((size_t)f * md.V + v) * 3;
    o[0] = acc[0] + tr[0]; o[1] = acc[1] + tr[1]; o[2] = acc[2] + tr[2];
}

// ---- LDS layout of the chain kernel ------------------------------------------------------------
int pick_nblk(int n, bool xt = false) {
    const int opts[5] = {2, 4, 5, 7, 8};
    const int opts_xt[4] = {5, 8, 10, 13};   // instantiations of the extended variant (chain_solve.hip)
    if (xt) { for (int o : opts_xt) if (o * 16 >= n + 1) return o; return -1; }
    for (int o : opts) if (o * 16 >= n + 1) return o;   // +1: the right-hand side rides along as row n (ldl_solve)
    return -1;
}

ChainLayout make_layout(const moshii_model_s* m, int Mmax, int Nvmax, int NWmax, int npose, int G, int nmax, int nkfmax, int Tm, int nblk = 0, int nhj = 0,
                        int nshape = 0) {
    ChainLayout ly;
    memset(&ly, 0, sizeof(ly));
    const int K = m->K, NP = m->NP, P = m->P;
    if (nblk <= 0) nblk = pick_nblk(nmax);
    const int LDJ = nblk * 16;
    ly.Mmax = Mmax; ly.Nvmax = Nvmax; ly.NWmax = NWmax; ly.nmax = nmax; ly.Tm = Tm; ly.nkfmax = nkfmax; ly.LDJ = LDJ; ly.nhj = nhj;
    int off = MOSHII_KC_DOUBLES;   // (the KernelCtx copy sits at the head of the LDS)
    auto take = [&](int nd) { int o = off; off += (nd + 1) & ~1; return o; };
    const int NPX = NP + nshape;   // free shape coefficients ride behind the pose variables
    ly.NPX = NPX;
    ly.o_pose = take(NPX); ly.o_trans = take(4); ly.o_pose_t = take(NPX); ly.o_trans_t = take(4);
    ly.o_vshp = take(nshape > 0 ? Nvmax * 3 : 0); ly.o_shp0 = take(nshape);
    ly.o_pose_prev = take(NP); ly.o_vtarget = take(NP); ly.o_fullpose = take(P);
    ly.o_feat = take(K * 9); ly.o_B = take(K * 28); ly.o_omega = take(K * 10); ly.o_Jl = take(K * 3); ly.o_Rw = take(K * 9); ly.o_tw = take(K * 3);
    ly.o_Rloc = take(K * 9); ly.o_acol = take(K * 9);
    ly.o_vconst = take(Nvmax * 3); ly.o_vposed = take(Nvmax * 3); ly.o_vpos = take(Nvmax * 3); ly.o_msim = take(Mmax * 3); ly.o_res = take(Mmax * 3);
    ly.o_xb = take(std::max(npose, 1) + 16);   // (+16: read unclamped in 16-row groups)
    ly.o_ell = take(std::max(8 * npose, 1) + 16); ly.o_score = take(std::max(G, 1));   // (ell: [2][4 waves][npose] + 16 zeros: read in 16-row groups)
    ly.o_px0 = take(std::max(npose, 1)); ly.o_ps0 = take(std::max(G, 1));
    ly.o_g = take(LDJ); ly.o_dsd = take(LDJ); ly.o_dgn = take(LDJ); ly.o_ddl = take(LDJ); ly.o_y = take(LDJ);
    ly.o_red = take(16); ly.o_scal = take(16);
    ly.o_anc = take(K);
    int io = 0;
    auto itake = [&](int ni) { int o = io; io += ni; return o; };
    ly.i_visidx = itake(Mmax); ly.i_colpid = itake(LDJ); ly.i_colprior = itake(LDJ); ly.i_pid2prior = itake(NP);
    ly.i_jointslot = itake(K); ly.i_kfree = itake(K); ly.i_colq = itake(NP); ly.i_ksum = itake(K); ly.i_kconst = itake(K);
    ly.i_total = io;
    ly.o_ints = take((io + 1) / 2);
    int t = 0;
    auto ttake = [&](int nd) { int o = t; t += (nd + 1) & ~1; return o; };
    ly.t_Jh = ttake(Tm * nhj * 9); ly.t_Jrow = ttake(3 * Tm * LDJ); ly.t_Lm = ttake(Tm * 30);
    ly.t_Trot = ttake(3 * Tm * 10); ly.t_xjs = ttake(3 * Tm * (NWmax * 4 + 2)); ly.t_rest = ttake(3 * Tm);   // (strides: assemble())
    ly.t_tjs = ttake((3 * Tm * (NWmax + 1) + 1) / 2);
    // packed factor + 64 per-lane trash words / zero word + the column broadcast buffer of ldl_solve; beyond 8 register blocks (extended variant)
    // the factor lives in global scratch and LDS keeps the broadcast buffer plus a 16-row panel
    // (ldl_big: a [LDJ][17] block column + nblk exchange tiles; its back-substitution lays two [16][LDJ] row buffers over them)
    const int chol = (nblk > 8) ? 66 + std::max(17 * LDJ + 256 * nblk, 32 * LDJ) + 4 : ((nblk <= 4) ? LDJ * (LDJ + 1) + 16 : (nmax + 1) * (nmax + 2) / 2) + 66 + 4 * LDJ + 4;   // (<= 4 blocks: the factor square, chain_solve.hip: ldl_square)
    ly.big_doubles = std::max(std::max(t, chol), 16 * 256);   // (16 x 256: the J^T J tile exchange, AReg::take)
    ly.o_big = take(ly.big_doubles);
    ly.total_doubles = off;
    return ly;
}

struct LaunchInfo { std::string name; int lds = 0; int threads = 0; } g_last;
std::mutex g_last_mutex;   // (moshii_joints_* may run on several host threads at once)
void note_launch(const std::string& name, int lds, int threads) {
    std::lock_guard<std::mutex> hold(g_last_mutex);
    g_last.name = name; g_last.lds = lds; g_last.threads = threads;
}

}  // namespace

// ================================================================================================
extern "C" {

const char* moshii_last_error(void) { return g_err.c_str(); }
int moshii_version(void) { return 107; }   // 101: moshii_stagei_desc grew by init_sq; 102: moshii_solve_opts by the joint-angle term; 103: moshii_lbs_forward_shape_*; 104: moshii_model_set_faces, moshii_vertex_normals_*, moshii_virtual_markers_*; 105: moshii_surface_distance_*, moshii_marker_surface_distance_*; 106: moshii_joints_*; 107: moshii_render_*, moshii_render_posed_* (include/moshii.h)
#ifndef MOSHII_SRC_HASH
#define MOSHII_SRC_HASH "unknown"
#endif
const char* moshii_source_hash(void) { return MOSHII_SRC_HASH; }

int moshii_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int moshii_set_device(int device) { HIP_TRY(hipSetDevice(device)); return MOSHII_OK; }

int moshii_device_multiprocessors(void) {
    int d = 0, n = 0;
    if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess) return 0;
    return n;
}

int moshii_model_create(const moshii_model_desc* d, moshii_model_t* out) {
    if (!d || !out) return fail(MOSHII_ERR_ARG, "null argument");
    if (d->K < 1 || d->K > MOSHII_MAXK) return fail(MOSHII_ERR_UNSUPPORTED, "K must be in [1,64]");
    if (moshii_device_count() < 1) return fail(MOSHII_ERR_NO_DEVICE, "no HIP device: libmoshii has no CPU path");
    const int P = 3 * d->K;
    if (d->body_dof < 3 || d->body_dof > P || d->body_dof % 3) return fail(MOSHII_ERR_ARG, "bad body_dof");
    const int nhf = P - d->body_dof;
    if ((d->hand_dof > 0) != (nhf > 0)) return fail(MOSHII_ERR_ARG, "hand_dof / body_dof mismatch");
    if (d->hand_dof > 0 && (!d->hands_mean || !d->selected_components)) return fail(MOSHII_ERR_ARG, "hand PCA arrays missing");
    std::unique_ptr<moshii_model_s> m(new moshii_model_s());   // (every failure below frees the handle and what it holds)
    m->V = d->V; m->K = d->K; m->NB = d->NB; m->P = P; m->body_dof = d->body_dof; m->hand_dof = d->hand_dof;
    m->nhand_full = nhf; m->NP = d->body_dof + d->hand_dof;
    m->parents.assign(d->parents, d->parents + d->K);
    m->depth.assign(d->K, 0);
    std::vector<unsigned long long> anc(d->K, 0ull);
    for (int j = 0; j < d->K; ++j) {
        int a = j, dep = 0;
        while (a >= 0) {
            anc[a] |= (1ull << j);
            const int p = m->parents[a];
            if (p >= a) return fail(MOSHII_ERR_ARG, "parents must precede children");
            a = p;
            if (a >= 0) ++dep;
        }
        m->depth[j] = dep;
        m->maxdepth = std::max(m->maxdepth, dep);
    }
    m->weights_host.assign(d->weights, d->weights + (size_t)d->V * d->K);
    const size_t V = d->V, K = d->K, nfeat = 9 * (K - 1);
    DevArena& mem = m->mem;
    m->d_vt = mem.upload(d->v_template, V * 3);
    m->d_shapedirs = mem.upload(d->shapedirs, V * 3 * d->NB);
    m->d_posedirs = mem.upload(d->posedirs, V * 3 * nfeat);
    m->d_weights = mem.upload(d->weights, V * K);
    m->d_Jreg = mem.upload(d->J_regressor, K * V);
    m->d_parents = mem.upload(m->parents.data(), K);
    {   // behind the depths: the joints sorted by depth ([K]) and where each depth starts ([maxdepth + 2]) -- the level-by-level walks of the kernels
        std::vector<int> dl(m->depth);
        for (int l = 0; l <= m->maxdepth; ++l) for (size_t j = 0; j < K; ++j) if (m->depth[j] == l) dl.push_back((int)j);
        int c = 0;
        for (int l = 0; l <= m->maxdepth + 1; ++l) { dl.push_back(c); for (size_t j = 0; j < K; ++j) c += (m->depth[j] == l) ? 1 : 0; }
        m->d_depth = mem.upload(dl.data(), dl.size());
    }
    m->d_anc = mem.upload(anc.data(), K);
    if (d->hand_dof > 0) {
        std::vector<int> lo(d->hand_dof), hi(d->hand_dof);
        for (int i = 0; i < d->hand_dof; ++i) {
            int l = nhf, h = 0;
            for (int c = 0; c < nhf; ++c)
                if (d->selected_components[(size_t)i * nhf + c] != 0.0) { l = std::min(l, c); h = std::max(h, c + 1); }
            if (l > h) { l = 0; h = 0; }
            lo[i] = l; hi[i] = h;
        }
        m->d_hands_mean = mem.upload(d->hands_mean, (size_t)nhf);
        m->d_comps = mem.upload(d->selected_components, (size_t)d->hand_dof * nhf);
        m->d_comp_lo = mem.upload(lo.data(), lo.size());
        m->d_comp_hi = mem.upload(hi.data(), hi.size());
        std::vector<int> clo(nhf), chi(nhf);
        for (int c = 0; c < nhf; ++c) {
            int l = d->hand_dof, h = 0;
            for (int i = 0; i < d->hand_dof; ++i)
                if (d->selected_components[(size_t)i * nhf + c] != 0.0) { l = std::min(l, i); h = std::max(h, i + 1); }
            if (l > h) { l = 0; h = 0; }
            clo[c] = l; chi[c] = h;
        }
        m->d_col_lo = mem.upload(clo.data(), clo.size());
        m->d_col_hi = mem.upload(chi.data(), chi.size());
    }
    m->d_vsh = mem.alloc<double>(V * 3);
    m->d_J = mem.alloc<double>(K * 3);
    if (!mem.ok()) return fail_mem(mem, "moshii_model_create");
    std::vector<double> zero(std::max(1, d->NB), 0.0);
    const int rc = moshii_model_set_betas(m.get(), zero.data(), d->NB);
    if (rc == MOSHII_OK) *out = m.release();
    return rc;
}

int moshii_model_destroy(moshii_model_t m) {
    if (!m) return MOSHII_OK;
    hipDeviceSynchronize();
    delete m;
    return MOSHII_OK;
}

int moshii_model_set_betas(moshii_model_t m, const double* betas, int32_t nb) {
    if (!m || (!betas && nb > 0)) return fail(MOSHII_ERR_ARG, "null argument");
    nb = std::min<int32_t>(nb, m->NB);
    DevArena tmp;
    const double* d_b = tmp.upload(betas, (size_t)std::max(nb, 0));
    if (!tmp.ok()) return fail_mem(tmp, "moshii_model_set_betas");
    const int tot = m->V * 3;
    hipLaunchKernelGGL(k_vshaped, dim3((tot + 255) / 256), dim3(256), 0, 0, m->V, m->NB, nb, m->d_vt, m->d_shapedirs, d_b, m->d_vsh);
    hipLaunchKernelGGL(k_joints, dim3(m->K), dim3(256), 0, 0, m->V, m->d_Jreg, m->d_vsh, m->d_J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    m->betas_set = true;
    m->l32_valid = false;
    return MOSHII_OK;
}

int moshii_model_set_free_shape(moshii_model_t m, int32_t start, int32_t count) {
    if (!m || start < 0 || count < 0 || start + count > m->NB) return fail(MOSHII_ERR_ARG, "free shape block outside shapedirs");
    if (count > 125) return fail(MOSHII_ERR_UNSUPPORTED, "at most 125 free shape coefficients");
    HIP_TRY(hipDeviceSynchronize());
    // the old block goes first; the new one is published only when it is whole: a failure leaves the handle without a block
    m->shape_mem.clear();
    m->d_JS = nullptr; m->shape_start = 0; m->nshape = 0;
    m->l32_valid = false;   // the f32 export's fragments and scratch sizes depend on the block
    if (count == 0) { m->shape_start = start; return MOSHII_OK; }
    DevArena fresh;
    double* d_JS = fresh.alloc<double>((size_t)m->K * count * 3);
    if (!fresh.ok()) return fail_mem(fresh, "moshii_model_set_free_shape");
    hipLaunchKernelGGL(k_shape_joints, dim3(m->K * count), dim3(256), 0, 0, m->V, m->NB, start, count, m->d_Jreg, m->d_shapedirs, d_JS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    m->shape_mem = std::move(fresh);
    m->d_JS = d_JS; m->shape_start = start; m->nshape = count;
    return MOSHII_OK;
}

int moshii_model_get_joints(moshii_model_t m, double* J_out) {
    if (!m || !J_out) return fail(MOSHII_ERR_ARG, "null argument");
    HIP_TRY(hipMemcpy(J_out, m->d_J, (size_t)m->K * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return MOSHII_OK;
}

// the f64 export's launch: shape = per-frame coefficients of the free block on the device, or null
static void launch_lbs_f64(moshii_model_t m, int F, const double* d_pose, const double* d_trans, const double* d_shape, double* d_out,
                           hipStream_t stream) {
    if (d_shape) {
        const size_t lds = (size_t)(m->P + m->K * 33) * sizeof(double);
        hipLaunchKernelGGL(k_lbs_f64<true>, dim3((m->V + 255) / 256, F), dim3(256), lds, stream, m->dev(), m->d_vsh, m->d_posedirs,
                           m->d_weights, d_pose, d_trans, d_out, m->d_shapedirs, m->NB, m->shape_start, d_shape);
    } else {
        const size_t lds = (size_t)(m->P + m->K * 30) * sizeof(double);
        hipLaunchKernelGGL(k_lbs_f64<false>, dim3((m->V + 255) / 256, F), dim3(256), lds, stream, m->dev(), m->d_vsh, m->d_posedirs,
                           m->d_weights, d_pose, d_trans, d_out, (const double*)nullptr, 0, 0, (const double*)nullptr);
    }
}

// implemented in lbs_forward.hip
int moshii_lbs32_prepare(moshii_model_t m);

}  // extern "C"

// ---- what the export entries share ----
namespace {
int need_shape_block(moshii_model_t m, const void* shape) {
    if (shape && m->nshape == 0) return fail(MOSHII_ERR_ARG, "shape coefficients without a block: call moshii_model_set_free_shape first");
    return MOSHII_OK;
}
int need_faces(moshii_model_t m, const char* name) {
    if (!m->d_vn_rows) return fail(MOSHII_ERR_ARG, std::string(name) + ": the model has no faces: call moshii_model_set_faces first");
    return MOSHII_OK;
}
template <class T> int need_l32(moshii_model_t m) {   // the f32 export works on its own copy of the model
    return (sizeof(T) == 4 && !m->l32_valid) ? moshii_lbs32_prepare(m) : MOSHII_OK;
}

// one export of nf frames, pointers on the device: the kernels of moshii_lbs_forward[_shape]_*
hipError_t export_batch(moshii_model_t m, int nf, const float* pose, const float* trans, const float* shape, float* out, hipStream_t stream) {
    ModelDev md = m->dev();
    const hipError_t e = moshii_launch_lbs_f32(stream, &md, nf, pose, trans, shape, out, &m->l32);
    if (e != hipSuccess) { moshii_lbs32_free(&m->l32); m->l32_valid = false; }   // (no half-grown copy is kept: the next call builds it again)
    return e;
}
hipError_t export_batch(moshii_model_t m, int nf, const double* pose, const double* trans, const double* shape, double* out, hipStream_t stream) {
    launch_lbs_f64(m, nf, pose, trans, shape, out, stream);
    return hipGetLastError();
}

// MOSHII_VM_BATCH (tests: batch boundaries with few frames), 0 = unset
int batch_override() {
    const char* es = getenv("MOSHII_VM_BATCH");
    return es ? std::max(1, atoi(es)) : 0;
}
}  // namespace

// shape: per-frame coefficients of the free block [F][nshape], or null (the frozen body)
template <class T>
static int lbs_forward_impl(moshii_model_t m, int32_t F, const T* pose, const T* trans, const T* shape, T* verts, uint32_t flags, void* stream_) {
    if (!m || !pose || !trans || !verts || F < 0) return fail(MOSHII_ERR_ARG, "bad argument");
    if (int rc = need_shape_block(m, shape)) return rc;
    if (F == 0) return MOSHII_OK;
    hipStream_t stream = (hipStream_t)stream_;
    Staging st(flags, stream);
    const T* d_pose = st.in(pose, (size_t)F * m->NP);
    const T* d_trans = st.in(trans, (size_t)F * 3);
    const T* d_shape = st.in(shape, (size_t)F * m->nshape);
    T* d_out = st.out(verts, (size_t)F * m->V * 3);
    if (!st.ok()) return fail_mem(st, "moshii_lbs_forward");
    if (int rc = need_l32<T>(m)) return rc;   // (behind the staging: a call that cannot stage its buffers builds nothing)
    HIP_TRY(export_batch(m, F, d_pose, d_trans, d_shape, d_out, stream));
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

template <class T>
static int vertex_normals_impl(moshii_model_t m, int32_t F, const T* verts, T* normals, uint32_t flags, void* stream_, const char* name) {
    if (!m || !verts || !normals || F < 0) return fail(MOSHII_ERR_ARG, std::string(name) + ": bad argument");
    if (int rc = need_faces(m, name)) return rc;
    if (F == 0) return MOSHII_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)F * m->V * 3;
    Staging st(flags, stream);
    const T* d_in = st.in(verts, n);
    T* d_out = st.out(normals, n);
    if (!st.ok()) return fail_mem(st, name);
    const char* which = "";
    int lds = 0, threads = 0;
    HIP_TRY(moshii_launch_vertex_normals(stream, m->V, F, sizeof(T) == 8, d_in, d_out, m->d_vn_rows, m->d_vn_pairs, m->vn_w16, &which, &lds, &threads));
    note_launch(which, lds, threads);
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

// The meshes exist only in the handle's scratch, a batch of frames at a time: export (the kernels of moshii_lbs_forward[_shape]_*, so
// the same vertices bit for bit as that call gives for the batch's frames), then the normals of the M marker vertices alone.
template <class T>
static int virtual_markers_impl(moshii_model_t m, int32_t F, const T* pose, const T* trans, const T* shape, int32_t M, const int32_t* vids,
                                const T* dist, T* markers, T* mnormals, uint32_t flags, void* stream_, const char* name) {
    if (!m || !pose || !trans || !vids || !dist || !markers || F < 0 || M < 1) return fail(MOSHII_ERR_ARG, std::string(name) + ": bad argument");
    if (int rc = need_shape_block(m, shape)) return rc;
    if (int rc = need_faces(m, name)) return rc;
    for (int i = 0; i < M; ++i) if (vids[i] < 0 || vids[i] >= m->V) return fail(MOSHII_ERR_ARG, std::string(name) + ": marker vertex id outside [0, V)");
    if (F == 0) return MOSHII_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = need_l32<T>(m)) return rc;
    const export_plan::Batch bp = export_plan::plan_batch((size_t)m->V * 3 * sizeof(T), F, M, sizeof(T) == 8, batch_override());
    if (int rc = m->vmscratch.reserve(bp.vm_bytes)) return rc;   // (waits for the call before this one)
    T* d_mesh = reinterpret_cast<T*>(m->vmscratch.ptr);
    int* d_vids = reinterpret_cast<int*>(m->vmscratch.ptr + bp.off_vids);
    double* d_dist = reinterpret_cast<double*>(m->vmscratch.ptr + bp.off_dist);
    std::vector<double> dist64(dist, dist + M);
    HIP_TRY(hipMemcpy(d_vids, vids, (size_t)M * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_dist, dist64.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice));
    const size_t nout = (size_t)F * M * 3;
    Staging st(flags, stream);
    const T* d_pose = st.in(pose, (size_t)F * m->NP);
    const T* d_trans = st.in(trans, (size_t)F * 3);
    const T* d_shape = st.in(shape, (size_t)F * m->nshape);
    T* d_out = st.out(markers, nout);
    T* d_nrm = st.out(mnormals, nout);
    if (!st.ok()) return fail_mem(st, name);
    m->vmscratch.used = true; m->vmscratch.last_stream = stream;
    for (long long f0 = 0; f0 < F; f0 += bp.batch) {
        const int nf = (int)std::min<long long>(bp.batch, F - f0);
        HIP_TRY(export_batch(m, nf, d_pose + (size_t)f0 * m->NP, d_trans + (size_t)f0 * 3,
                             d_shape ? d_shape + (size_t)f0 * m->nshape : (const T*)nullptr, d_mesh, stream));
        HIP_TRY(moshii_launch_marker_normals(stream, m->V, nf, M, sizeof(T) == 8, d_mesh, d_vids, d_dist, d_out + (size_t)f0 * M * 3,
                                             d_nrm ? d_nrm + (size_t)f0 * M * 3 : (T*)nullptr, m->d_vn_rows, m->d_vn_pairs, m->vn_w16));
    }
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

// ---- signed point-to-mesh distance (version 105) ----
namespace {
const char* sd_check(moshii_model_t m, int32_t F, int32_t N, const void* dist) {
    if (!m) return "null model";
    if (F < 0 || N < 0) return "negative F or N";
    if (!dist) return "dist is null";
    return nullptr;
}
}  // namespace

// verts / points / outputs on the device; `face` may be null (the winners then go to d_win)
template <class T>
static int surface_distance_launch(moshii_model_t m, int F, const T* d_verts, int N, const T* d_points, T* d_dist, int* d_face, int* d_part,
                                   T* d_near, int* d_win, hipStream_t stream) {
    const char* which = "";
    int lds = 0, threads = 0;
    HIP_TRY(moshii_launch_surface_distance(stream, m->V, m->n_faces, F, N, sizeof(T) == 8, d_verts, d_points, m->d_sd_tris, m->vn_w16, m->d_vn_rows,
                                           m->d_vn_pairs, d_dist, d_face ? d_face : d_win, d_part, d_near, &which, &lds, &threads));
    note_launch(which, lds, threads);
    return MOSHII_OK;
}

template <class T>
static int surface_distance_impl(moshii_model_t m, int32_t F, const T* verts, int32_t N, const T* points, T* dist, int32_t* face, int32_t* part,
                                 T* nearest, uint32_t flags, void* stream_, const char* name) {
    if (const char* bad = sd_check(m, F, N, dist)) return fail(MOSHII_ERR_ARG, std::string(name) + ": " + bad);
    if (int rc = need_faces(m, name)) return rc;
    if (F == 0 || N == 0) return MOSHII_OK;
    if (!verts || !points) return fail(MOSHII_ERR_ARG, std::string(name) + ": verts or points is null");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t nv = (size_t)F * m->V * 3, np = (size_t)F * N;
    Staging st(flags, stream);
    int* d_win = nullptr;   // the search's winners when the caller takes no `face`: the handle's scratch, or a temporary of this call
    if (!face && st.device()) {
        if (int rc = m->sdscratch.reserve(np * sizeof(int), stream)) return rc;   // (waits for the call before this one)
        d_win = reinterpret_cast<int*>(m->sdscratch.ptr);
    }
    const T* d_verts = st.in(verts, nv);
    const T* d_points = st.in(points, np * 3);
    T* d_dist = st.out(dist, np);
    int* d_face = st.out(face, np);
    if (!face && !st.device()) d_win = st.mem().alloc<int>(np);
    int* d_part = st.out(part, np);
    T* d_near = st.out(nearest, np * 3);
    if (!st.ok()) return fail_mem(st, name);
    if (int rc = surface_distance_launch(m, F, d_verts, N, d_points, d_dist, d_face, d_part, d_near, d_win, stream)) return rc;
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

// The meshes exist only in the handle's scratch, a batch of frames at a time, sized and exported as moshii_virtual_markers_* does;
// each batch's points meet their own frames' meshes there and only the F x N results leave.
template <class T>
static int marker_surface_distance_impl(moshii_model_t m, int32_t F, const T* pose, const T* trans, const T* shape, int32_t N, const T* points,
                                        T* dist, int32_t* face, int32_t* part, T* nearest, uint32_t flags, void* stream_, const char* name) {
    if (const char* bad = sd_check(m, F, N, dist)) return fail(MOSHII_ERR_ARG, std::string(name) + ": " + bad);
    if (int rc = need_shape_block(m, shape)) return rc;
    if (int rc = need_faces(m, name)) return rc;
    if (F == 0 || N == 0) return MOSHII_OK;
    if (!pose || !trans || !points) return fail(MOSHII_ERR_ARG, std::string(name) + ": pose, trans or points is null");
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = need_l32<T>(m)) return rc;
    const export_plan::Batch bp = export_plan::plan_batch((size_t)m->V * 3 * sizeof(T), F, N, sizeof(T) == 8, batch_override());
    if (int rc = m->vmscratch.reserve(face ? bp.sd_bytes_face : bp.sd_bytes)) return rc;   // (waits for the call before this one)
    T* d_mesh = reinterpret_cast<T*>(m->vmscratch.ptr);
    int* d_win = face ? (int*)nullptr : reinterpret_cast<int*>(m->vmscratch.ptr + bp.off_win);
    const size_t np = (size_t)F * N;
    Staging st(flags, stream);
    const T* d_pose = st.in(pose, (size_t)F * m->NP);
    const T* d_trans = st.in(trans, (size_t)F * 3);
    const T* d_shape = st.in(shape, (size_t)F * m->nshape);
    const T* d_points = st.in(points, np * 3);
    T* d_dist = st.out(dist, np);
    int* d_face = st.out(face, np);
    int* d_part = st.out(part, np);
    T* d_near = st.out(nearest, np * 3);
    if (!st.ok()) return fail_mem(st, name);
    m->vmscratch.used = true; m->vmscratch.last_stream = stream;
    for (long long f0 = 0; f0 < F; f0 += bp.batch) {
        const int nf = (int)std::min<long long>(bp.batch, F - f0);
        const size_t at = (size_t)f0 * N;
        HIP_TRY(export_batch(m, nf, d_pose + (size_t)f0 * m->NP, d_trans + (size_t)f0 * 3,
                             d_shape ? d_shape + (size_t)f0 * m->nshape : (const T*)nullptr, d_mesh, stream));
        if (int rc = surface_distance_launch(m, nf, (const T*)d_mesh, N, d_points + at * 3, d_dist + at, d_face ? d_face + at : (int*)nullptr,
                                             d_part ? d_part + at : (int*)nullptr, d_near ? d_near + at * 3 : (T*)nullptr, d_win, stream)) return rc;
    }
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

// ---- posed joints and world joint rotations (version 106) ----
// Nothing of the handle is written: no scratch, no f32 copy, no faces -- the kernel reads the model arrays and the caller's buffers, so
// the call may run beside an export of the same handle on another stream.
template <class T>
static int joints_impl(moshii_model_t m, int32_t F, const T* pose, const T* trans, const T* shape, T* joints, T* rot, uint32_t flags,
                       void* stream_, const char* name) {
    if (!m) return fail(MOSHII_ERR_ARG, std::string(name) + ": null model");
    if (F < 0) return fail(MOSHII_ERR_ARG, std::string(name) + ": negative F");
    if (!joints) return fail(MOSHII_ERR_ARG, std::string(name) + ": joints is null");
    if (!m->betas_set) return fail(MOSHII_ERR_ARG, std::string(name) + ": moshii_model_set_betas has not been called");
    if (int rc = need_shape_block(m, shape)) return rc;
    if (F == 0) return MOSHII_OK;
    if (!pose || !trans) return fail(MOSHII_ERR_ARG, std::string(name) + ": pose or trans is null");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t nj = (size_t)F * m->K * 3;
    Staging st(flags, stream);
    const T* d_pose = st.in(pose, (size_t)F * m->NP);
    const T* d_trans = st.in(trans, (size_t)F * 3);
    const T* d_shape = st.in(shape, (size_t)F * m->nshape);
    T* d_joints = st.out(joints, nj);
    T* d_rot = st.out(rot, nj * 3);
    if (!st.ok()) return fail_mem(st, name);
    const ModelDev md = m->dev();
    const char* which = "";
    int threads = 0;
    HIP_TRY(moshii_launch_joints(stream, &md, F, sizeof(T) == 8, d_pose, d_trans, d_shape, d_joints, d_rot, &which, &threads));
    note_launch(which, 0, threads);
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

// ---- shaded previews (version 107) ----
namespace {
const char* render_check(moshii_model_t m, int32_t F, int32_t N, const void* points, const moshii_render_opts* o, const void* rgb,
                         const void* ids, const void* depth) {
    if (!m) return "null model";
    if (F < 0 || N < 0) return "negative F or N";
    if (!o) return "opts is null";
    if (!o->cameras) return "opts->cameras is null";
    if (!rgb && !ids && !depth) return "rgb, ids and depth are all null";
    if (o->width < 1 || o->width > 4096 || o->height < 1 || o->height > 4096) return "width and height must be within 1 .. 4096";
    if (o->n_cameras != 1 && o->n_cameras != F) return "n_cameras must be 1 or F";
    if (N > 0 && (!points || !o->point_rgb || !o->point_radius)) return "N > 0 needs points, point_rgb and point_radius";
    if (!(o->ambient >= 0.0 && o->ambient <= 1.0)) return "ambient must be within 0 .. 1";
    return nullptr;
}
}  // namespace

// Both entries: a batch of frames at a time from the handle's scratch (export_plan.h: plan_render) -- the batch's vertex normals (the
// kernels of moshii_vertex_normals_*), its projected records, then one workgroup a tile and frame.  verts: the caller's meshes
// (moshii_render_*), or null and pose / trans / shape, exported into the scratch first as moshii_virtual_markers_* does.
template <class T>
static int render_impl(moshii_model_t m, int32_t F, const T* verts, const T* pose, const T* trans, const T* shape, bool posed, int32_t N,
                       const T* points, const moshii_render_opts* o, uint8_t* rgb, int32_t* ids, float* depth, uint32_t flags, void* stream_,
                       const char* name) {
    if (const char* bad = render_check(m, F, N, points, o, rgb, ids, depth)) return fail(MOSHII_ERR_ARG, std::string(name) + ": " + bad);
    if (posed) if (int rc = need_shape_block(m, shape)) return rc;
    if (int rc = need_faces(m, name)) return rc;
    if ((long long)m->n_faces + N > 0x7fffffffLL) return fail(MOSHII_ERR_UNSUPPORTED, std::string(name) + ": faces + points beyond the 31 bits of an id");
    if (F == 0) return MOSHII_OK;
    if (posed ? (!pose || !trans) : !verts) return fail(MOSHII_ERR_ARG, std::string(name) + (posed ? ": pose or trans is null" : ": verts is null"));
    hipStream_t stream = (hipStream_t)stream_;
    if (posed) if (int rc = need_l32<T>(m)) return rc;
    const int V = m->V, W = o->width, H = o->height;
    const size_t frame_bytes = (size_t)V * 3 * sizeof(T);
    const export_plan::RenderBatch bp = export_plan::plan_render(frame_bytes, F, V, N, o->n_cameras, posed, batch_override());
    if (int rc = m->vmscratch.reserve(bp.bytes)) return rc;   // (waits for the call before this one)
    char* base = m->vmscratch.ptr;
    T* d_mesh = reinterpret_cast<T*>(base);
    T* d_normals = reinterpret_cast<T*>(base + bp.off_normals);
    moshii_camera* d_cams = reinterpret_cast<moshii_camera*>(base + bp.off_cams);
    double* d_radius = reinterpret_cast<double*>(base + bp.off_radius);
    HIP_TRY(hipMemcpy(d_cams, o->cameras, (size_t)o->n_cameras * sizeof(moshii_camera), hipMemcpyHostToDevice));
    if (N > 0) {
        HIP_TRY(hipMemcpy(d_radius, o->point_radius, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(base + bp.off_prgb, o->point_rgb, (size_t)N * 3, hipMemcpyHostToDevice));
    }
    const size_t npix = (size_t)F * H * W;
    Staging st(flags, stream);
    const T* d_verts = posed ? (const T*)nullptr : st.in(verts, (size_t)F * V * 3);
    const T* d_pose = posed ? st.in(pose, (size_t)F * m->NP) : (const T*)nullptr;
    const T* d_trans = posed ? st.in(trans, (size_t)F * 3) : (const T*)nullptr;
    const T* d_shape = posed ? st.in(shape, (size_t)F * m->nshape) : (const T*)nullptr;
    const T* d_points = N > 0 ? st.in(points, (size_t)F * N * 3) : (const T*)nullptr;
    uint8_t* d_rgb = st.out(rgb, npix * 3);
    int32_t* d_ids = st.out(ids, npix);
    float* d_depth = st.out(depth, npix);
    if (!st.ok()) return fail_mem(st, name);
    m->vmscratch.used = true; m->vmscratch.last_stream = stream;
    RenderArgs A;
    memset(&A, 0, sizeof(A));
    A.V = V; A.NF = m->n_faces; A.N = N; A.W = W; A.H = H; A.w16 = m->vn_w16;
    A.tris = m->d_sd_tris;
    A.rec = reinterpret_cast<const RenderVertex*>(base + bp.off_rec);
    A.mrec = reinterpret_cast<const RenderMarker*>(base + bp.off_mrec);
    A.prgb = reinterpret_cast<const unsigned char*>(base + bp.off_prgb);
    for (int i = 0; i < 3; ++i) { A.body[i] = o->body_rgb[i]; A.bg[i] = o->bg_rgb[i]; }
    A.ambient = o->ambient;
    const char* which = "";
    int lds = 0, threads = 0;
    for (long long f0 = 0; f0 < F; f0 += bp.batch) {
        const int nf = (int)std::min<long long>(bp.batch, F - f0);
        const T* mesh = posed ? d_mesh : d_verts + (size_t)f0 * V * 3;
        if (posed)
            HIP_TRY(export_batch(m, nf, d_pose + (size_t)f0 * m->NP, d_trans + (size_t)f0 * 3,
                                 d_shape ? d_shape + (size_t)f0 * m->nshape : (const T*)nullptr, d_mesh, stream));
        HIP_TRY(moshii_launch_vertex_normals(stream, V, nf, sizeof(T) == 8, mesh, d_normals, m->d_vn_rows, m->d_vn_pairs, m->vn_w16, nullptr, nullptr, nullptr));
        const size_t p0 = (size_t)f0 * H * W;
        A.rgb = d_rgb ? d_rgb + p0 * 3 : nullptr;
        A.ids = d_ids ? d_ids + p0 : nullptr;
        A.depth = d_depth ? d_depth + p0 : nullptr;
        const int stride = o->n_cameras == 1 ? 0 : 1;
        HIP_TRY(moshii_launch_render(stream, nf, sizeof(T) == 8, mesh, d_normals, d_points ? d_points + (size_t)f0 * N * 3 : (const T*)nullptr, d_radius,
                                     d_cams + (stride ? f0 : 0), stride, &A, &which, &lds, &threads));
    }
    note_launch(which, lds, threads);
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

extern "C" {

int moshii_render_f32(moshii_model_t m, int32_t F, const float* verts, int32_t N, const float* points, const moshii_render_opts* opts,
                      uint8_t* rgb, int32_t* ids, float* depth, uint32_t flags, void* stream) {
    return render_impl<float>(m, F, verts, nullptr, nullptr, nullptr, false, N, points, opts, rgb, ids, depth, flags, stream, "moshii_render_f32");
}
int moshii_render_f64(moshii_model_t m, int32_t F, const double* verts, int32_t N, const double* points, const moshii_render_opts* opts,
                      uint8_t* rgb, int32_t* ids, float* depth, uint32_t flags, void* stream) {
    return render_impl<double>(m, F, verts, nullptr, nullptr, nullptr, false, N, points, opts, rgb, ids, depth, flags, stream, "moshii_render_f64");
}
int moshii_render_posed_f32(moshii_model_t m, int32_t F, const float* pose, const float* trans, const float* shape, int32_t N, const float* points,
                            const moshii_render_opts* opts, uint8_t* rgb, int32_t* ids, float* depth, uint32_t flags, void* stream) {
    return render_impl<float>(m, F, nullptr, pose, trans, shape, true, N, points, opts, rgb, ids, depth, flags, stream, "moshii_render_posed_f32");
}
int moshii_render_posed_f64(moshii_model_t m, int32_t F, const double* pose, const double* trans, const double* shape, int32_t N, const double* points,
                            const moshii_render_opts* opts, uint8_t* rgb, int32_t* ids, float* depth, uint32_t flags, void* stream) {
    return render_impl<double>(m, F, nullptr, pose, trans, shape, true, N, points, opts, rgb, ids, depth, flags, stream, "moshii_render_posed_f64");
}

int moshii_lbs_forward_f64(moshii_model_t m, int32_t F, const double* pose, const double* trans, double* verts,
                           uint32_t flags, void* stream) {
    return lbs_forward_impl<double>(m, F, pose, trans, nullptr, verts, flags, stream);
}
int moshii_lbs_forward_shape_f64(moshii_model_t m, int32_t F, const double* pose, const double* trans, const double* shape,
                                 double* verts, uint32_t flags, void* stream) {
    return lbs_forward_impl(m, F, pose, trans, shape, verts, flags, stream);
}
int moshii_lbs_forward_f32(moshii_model_t m, int32_t F, const float* pose, const float* trans, float* verts,
                           uint32_t flags, void* stream) {
    return lbs_forward_impl<float>(m, F, pose, trans, nullptr, verts, flags, stream);
}
int moshii_lbs_forward_shape_f32(moshii_model_t m, int32_t F, const float* pose, const float* trans, const float* shape,
                                 float* verts, uint32_t flags, void* stream) {
    return lbs_forward_impl(m, F, pose, trans, shape, verts, flags, stream);
}

// ---- faces, vertex normals, virtual markers (version 104) ----
int moshii_model_set_faces(moshii_model_t m, int32_t n_faces, const int32_t* faces) {
    if (!m || n_faces < 0 || (n_faces > 0 && !faces)) return fail(MOSHII_ERR_ARG, "moshii_model_set_faces: bad argument");
    if (n_faces > 0x3fffffff) return fail(MOSHII_ERR_UNSUPPORTED, "moshii_model_set_faces: at most 2^30 - 1 faces (32-bit row offsets)");
    const int V = m->V;
    for (size_t i = 0; i < (size_t)n_faces * 3; ++i)
        if (faces[i] < 0 || faces[i] >= V) return fail(MOSHII_ERR_ARG, "moshii_model_set_faces: vertex id outside [0, V)");
    HIP_TRY(hipDeviceSynchronize());
    m->face_mem.clear();
    m->d_vn_rows = nullptr; m->d_vn_pairs = nullptr; m->d_sd_tris = nullptr;
    m->n_faces = 0;
    if (n_faces == 0) return MOSHII_OK;
    // vertex -> incident corners: for vertex v of face (a, b, c) the other two in cyclic order, (p - v) x (q - v) = the face's scaled
    // normal; a face that names a vertex twice has none and is left out
    std::vector<unsigned> rows((size_t)V + 1, 0u);
    auto good = [&](int f) { const int32_t* t = faces + (size_t)f * 3; return t[0] != t[1] && t[1] != t[2] && t[0] != t[2]; };
    for (int f = 0; f < n_faces; ++f) if (good(f)) for (int c = 0; c < 3; ++c) ++rows[(size_t)faces[(size_t)f * 3 + c] + 1];
    for (int v = 0; v < V; ++v) rows[v + 1] += rows[v];
    const size_t nc = rows[V];
    const bool w16 = V <= 65535;        // 16-bit pairs: half the table, and every frame reads all of it
    std::vector<unsigned> pairs(std::max<size_t>(nc * (w16 ? 1 : 2), 1), 0u), fill(rows.begin(), rows.end() - 1);
    for (int f = 0; f < n_faces; ++f) {
        if (!good(f)) continue;
        const int32_t* t = faces + (size_t)f * 3;
        for (int c = 0; c < 3; ++c) {
            const unsigned p = (unsigned)t[(c + 1) % 3], q = (unsigned)t[(c + 2) % 3];
            const size_t at = fill[t[c]]++;
            if (w16) pairs[at] = p | (q << 16);
            else { pairs[2 * at] = p; pairs[2 * at + 1] = q; }
        }
    }
    // the triangles as the distance search reads them (every face, the degenerate ones too: face ids are the caller's)
    std::vector<unsigned> tris((size_t)n_faces * (w16 ? 2 : 3));
    for (size_t f = 0; f < (size_t)n_faces; ++f) {
        const int32_t* t = faces + f * 3;
        if (w16) { tris[2 * f] = (unsigned)t[0] | ((unsigned)t[1] << 16); tris[2 * f + 1] = (unsigned)t[2]; }
        else for (int c = 0; c < 3; ++c) tris[3 * f + c] = (unsigned)t[c];
    }
    // every part uploaded before any is published: a failure leaves the handle without a table, never with half of one
    DevArena fresh;
    unsigned* d_rows = fresh.upload(rows.data(), rows.size());
    unsigned* d_pairs = fresh.upload(pairs.data(), pairs.size());
    unsigned* d_tris = fresh.upload(tris.data(), tris.size());
    if (!fresh.ok()) return fail_mem(fresh, "moshii_model_set_faces");
    m->face_mem = std::move(fresh);
    m->d_vn_rows = d_rows; m->d_vn_pairs = d_pairs; m->d_sd_tris = d_tris;
    m->n_faces = n_faces;
    m->vn_w16 = w16 ? 1 : 0;
    return MOSHII_OK;
}

int moshii_vertex_normals_f32(moshii_model_t m, int32_t F, const float* verts, float* normals, uint32_t flags, void* stream) {
    return vertex_normals_impl(m, F, verts, normals, flags, stream, "moshii_vertex_normals_f32");
}
int moshii_vertex_normals_f64(moshii_model_t m, int32_t F, const double* verts, double* normals, uint32_t flags, void* stream) {
    return vertex_normals_impl(m, F, verts, normals, flags, stream, "moshii_vertex_normals_f64");
}
int moshii_virtual_markers_f32(moshii_model_t m, int32_t F, const float* pose, const float* trans, const float* shape, int32_t M,
                               const int32_t* vids, const float* dist, float* markers, float* marker_normals, uint32_t flags, void* stream) {
    return virtual_markers_impl(m, F, pose, trans, shape, M, vids, dist, markers, marker_normals, flags, stream, "moshii_virtual_markers_f32");
}
int moshii_virtual_markers_f64(moshii_model_t m, int32_t F, const double* pose, const double* trans, const double* shape, int32_t M,
                               const int32_t* vids, const double* dist, double* markers, double* marker_normals, uint32_t flags, void* stream) {
    return virtual_markers_impl(m, F, pose, trans, shape, M, vids, dist, markers, marker_normals, flags, stream, "moshii_virtual_markers_f64");
}
int moshii_surface_distance_f32(moshii_model_t m, int32_t F, const float* verts, int32_t N, const float* points, float* dist, int32_t* face,
                                int32_t* part, float* nearest, uint32_t flags, void* stream) {
    return surface_distance_impl(m, F, verts, N, points, dist, face, part, nearest, flags, stream, "moshii_surface_distance_f32");
}
int moshii_surface_distance_f64(moshii_model_t m, int32_t F, const double* verts, int32_t N, const double* points, double* dist, int32_t* face,
                                int32_t* part, double* nearest, uint32_t flags, void* stream) {
    return surface_distance_impl(m, F, verts, N, points, dist, face, part, nearest, flags, stream, "moshii_surface_distance_f64");
}
int moshii_marker_surface_distance_f32(moshii_model_t m, int32_t F, const float* pose, const float* trans, const float* shape, int32_t N,
                                       const float* points, float* dist, int32_t* face, int32_t* part, float* nearest, uint32_t flags, void* stream) {
    return marker_surface_distance_impl(m, F, pose, trans, shape, N, points, dist, face, part, nearest, flags, stream, "moshii_marker_surface_distance_f32");
}
int moshii_marker_surface_distance_f64(moshii_model_t m, int32_t F, const double* pose, const double* trans, const double* shape, int32_t N,
                                       const double* points, double* dist, int32_t* face, int32_t* part, double* nearest, uint32_t flags, void* stream) {
    return marker_surface_distance_impl(m, F, pose, trans, shape, N, points, dist, face, part, nearest, flags, stream, "moshii_marker_surface_distance_f64");
}
int moshii_joints_f32(moshii_model_t m, int32_t F, const float* pose, const float* trans, const float* shape, float* joints, float* rot,
                      uint32_t flags, void* stream) {
    return joints_impl(m, F, pose, trans, shape, joints, rot, flags, stream, "moshii_joints_f32");
}
int moshii_joints_f64(moshii_model_t m, int32_t F, const double* pose, const double* trans, const double* shape, double* joints, double* rot,
                      uint32_t flags, void* stream) {
    return joints_impl(m, F, pose, trans, shape, joints, rot, flags, stream, "moshii_joints_f64");
}

int moshii_prior_create(int32_t G, int32_t npose, const double* means, const double* chols, const double* weights,
                        moshii_prior_t* out) {
    if (!means || !chols || !weights || !out || G < 1 || npose < 1) return fail(MOSHII_ERR_ARG, "bad argument");
    if (npose > 127) return fail(MOSHII_ERR_UNSUPPORTED, "prior npose > 127 (the chain kernel takes a prior's columns two per lane)");
    if (moshii_device_count() < 1) return fail(MOSHII_ERR_NO_DEVICE, "no HIP device: libmoshii has no CPU path");
    std::unique_ptr<moshii_prior_s> p(new moshii_prior_s());
    p->G = G; p->npose = npose;
    const size_t nn = (size_t)npose * npose;
    std::vector<double> half((size_t)G * nn), nlw(G), cn(G), lower((size_t)G * nn, 0.0);   // lower: the factors with explicit zeros above the
    for (int g = 0; g < G; ++g) {                                                    // diagonal (the chain kernel reads whole rows)
        const double* L = chols + g * nn;
        for (int i = 0; i < npose; ++i)
            for (int j = 0; j <= i; ++j) lower[g * nn + (size_t)i * npose + j] = L[(size_t)i * npose + j];
        for (int i = 0; i < npose; ++i)
            for (int j = 0; j <= i; ++j) {
                double s = 0.0;
                for (int a = 0; a <= j; ++a) s += L[(size_t)i * npose + a] * L[(size_t)j * npose + a];   // (L L^T)_ij, L lower
                half[g * nn + (size_t)i * npose + j] = 0.5 * s;
                half[g * nn + (size_t)j * npose + i] = 0.5 * s;
            }
        nlw[g] = -std::log(weights[g]);
        // |L|_2 <= min(|L|_F, sqrt(|L|_1 |L|_inf)); a hair above, so that rounding here cannot make the bound too small
        double fro = 0.0, n1 = 0.0, ninf = 0.0;
        std::vector<double> colsum(npose, 0.0);
        for (int i = 0; i < npose; ++i) {
            double rs = 0.0;
            for (int j = 0; j <= i; ++j) { const double v = std::fabs(L[(size_t)i * npose + j]); fro += v * v; rs += v; colsum[j] += v; }
            ninf = std::max(ninf, rs);
        }
        for (int j = 0; j < npose; ++j) n1 = std::max(n1, colsum[j]);
        cn[g] = std::min(std::sqrt(fro), std::sqrt(n1 * ninf)) * 0.70710678118654757 * (1.0 + 1e-12);
    }
    // (means and factors carry 16 entries / rows of zero padding: the chain kernel reads whole 16-row groups unclamped)
    std::vector<double> means_p((size_t)G * npose + 16, 0.0);
    std::copy(means, means + (size_t)G * npose, means_p.begin());
    lower.resize((size_t)G * nn + (size_t)16 * npose, 0.0);
    p->d_means = p->mem.upload(means_p.data(), means_p.size());
    p->d_chols = p->mem.upload(lower.data(), lower.size());
    p->d_halfprec = p->mem.upload(half.data(), half.size());
    p->d_neglogw = p->mem.upload(nlw.data(), nlw.size());
    p->d_cnorm = p->mem.upload(cn.data(), cn.size());
    if (!p->mem.ok()) return fail_mem(p->mem, "moshii_prior_create");
    *out = p.release();
    return MOSHII_OK;
}

int moshii_prior_destroy(moshii_prior_t p) {
    if (!p) return MOSHII_OK;
    hipDeviceSynchronize();
    delete p;
    return MOSHII_OK;
}

int moshii_attach_create(moshii_model_t m, int32_t M, const int32_t* closest, const double* coef, moshii_attach_t* out) {
    if (!m || !closest || !coef || !out || M < 1) return fail(MOSHII_ERR_ARG, "bad argument");
    if (M > 128) return fail(MOSHII_ERR_UNSUPPORTED, "at most 128 latent markers");
    std::unique_ptr<moshii_attach_s> a(new moshii_attach_s());
    a->model = m; a->M = M; a->Nv = 3 * M; a->Nvp = (a->Nv + 7) & ~7;
    std::vector<int> vids(a->Nv);
    int NW = 1;
    for (int i = 0; i < a->Nv; ++i) {
        vids[i] = closest[i];
        if (vids[i] < 0 || vids[i] >= m->V) return fail(MOSHII_ERR_ARG, "vertex id out of range");
        int c = 0;
        for (int j = 0; j < m->K; ++j) if (m->weights_host[(size_t)vids[i] * m->K + j] != 0.0) ++c;
        NW = std::max(NW, c);
    }
    a->NW = NW;
    std::vector<int> wj((size_t)a->Nv * NW, 0);
    std::vector<double> ww((size_t)a->Nv * NW, 0.0);
    for (int i = 0; i < a->Nv; ++i) {
        int c = 0;
        for (int j = 0; j < m->K; ++j) {
            const double w = m->weights_host[(size_t)vids[i] * m->K + j];
            if (w != 0.0) { wj[(size_t)i * NW + c] = j; ww[(size_t)i * NW + c] = w; ++c; }
        }
    }
    DevArena& mem = a->mem;
    a->d_vids = mem.upload(vids.data(), vids.size());
    a->d_wj = mem.upload(wj.data(), wj.size());
    a->d_ww = mem.upload(ww.data(), ww.size());
    a->d_coef = mem.upload(coef, (size_t)M * 3);
    a->d_vsh = mem.alloc<double>((size_t)a->Nv * 3);
    const size_t npt = (size_t)(m->K - 1) * 27 * a->Nvp;
    a->d_Pt = mem.alloc<double>(npt);
    a->d_Pj = mem.alloc<double>((size_t)(m->K - 1) * 3 * 14 * M * 2);
    if (!mem.ok()) return fail_mem(mem, "moshii_attach_create");
    const int blocks = (int)std::min<size_t>(4096, std::max<size_t>((npt + 255) / 256, (size_t)(a->Nv * 3 + 255) / 256));
    hipLaunchKernelGGL(k_pack_attach, dim3(std::max(blocks, 1)), dim3(256), 0, 0, a->Nv, a->Nvp, m->K, a->d_vids, m->d_posedirs,
                       m->d_vsh, a->d_Pt, a->d_Pj, a->d_vsh);
    HIP_TRY(hipGetLastError());
    if (m->nshape > 0) {   // rows of the free shape block (moshii_model_set_free_shape)
        a->nshape = m->nshape;
        const size_t ns = (size_t)m->nshape * 3 * a->Nvp;
        a->d_Ssh = mem.alloc<double>(ns);
        if (!mem.ok()) return fail_mem(mem, "moshii_attach_create");
        hipLaunchKernelGGL(k_pack_shape, dim3((unsigned)std::min<size_t>(4096, (ns + 255) / 256)), dim3(256), 0, 0, a->Nv, a->Nvp, m->NB,
                           m->shape_start, m->nshape, a->d_vids, m->d_shapedirs, a->d_Ssh);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    AttachDev& av = a->host_view;
    av.M = M; av.Nv = a->Nv; av.Nvp = a->Nvp; av.NW = NW;
    av.vsh = as_gp(a->d_vsh); av.Pt = as_gp(a->d_Pt); av.Pj = as_gp(a->d_Pj); av.wj = as_gp(a->d_wj); av.ww = as_gp(a->d_ww);
    av.coef = as_gp(a->d_coef); av.Ssh = as_gp(a->d_Ssh);
    a->d_self = mem.upload(&av, 1);
    if (!mem.ok()) return fail_mem(mem, "moshii_attach_create");
    *out = a.release();
    return MOSHII_OK;
}

int moshii_attach_destroy(moshii_attach_t a) {
    if (!a) return MOSHII_OK;
    hipDeviceSynchronize();
    delete a;
    return MOSHII_OK;
}

int moshii_attach_markers(moshii_attach_t a, int32_t F, const double* pose, const double* trans, double* markers) {
    if (!a || !pose || !trans || !markers || F < 0) return fail(MOSHII_ERR_ARG, "bad argument");
    if (F == 0) return MOSHII_OK;
    moshii_model_t m = a->model;
    ChainLayout ly = make_layout(m, a->M, a->Nv, a->NW, 0, 0, 16, 1, 1);
    Staging st(MOSHII_BUFFERS_HOST, nullptr);   // (host buffers, the null stream)
    const double* d_pose = st.in(pose, (size_t)F * m->NP);
    const double* d_trans = st.in(trans, (size_t)F * 3);
    double* d_out = st.out(markers, (size_t)F * a->M * 3);
    if (!st.ok()) return fail_mem(st, "moshii_attach_markers");
    ModelDev md = m->dev();
    HIP_TRY(moshii_launch_markers(F, (size_t)ly.total_doubles * sizeof(double), 0, a->d_self, &md, &ly, d_pose, d_trans, d_out));
    HIP_TRY(st.finish());
    return MOSHII_OK;
}

}  // extern "C" (reopened below)

// ---- shared launch preparation for moshii_chain_solve / moshii_sequence_solve -----------------------
// (the arithmetic of the plan -- chunk table, group choice, exchange layout, repair scheduling -- is solve_plan.h)
namespace {
using solve_plan::Chunk;
using solve_plan::CoopLayout;
using solve_plan::coop_split;
static_assert(solve_plan::kThreads == MOSHII_TPB && solve_plan::kMaxGroup == MOSHII_COOP_MAXG, "solve_plan.h restates them");

struct LaunchCfg {
    int nblk = 0;
    int xt = 0;                 // extended kernel variant (jaw term / free shape block)
    int coop_g = 0;             // > 0: cooperative chains, this many workgroups per chain
    int coop_prior_rank = 0;
    double coop_prior_frac = 0.4;
    CoopLayout coop;            // cooperative chains: one chain's slice of the exchange buffer
    ChainLayout ly;
    size_t lds_bytes = 0;
    OptsDev od;
    PriorDev pd;
    ModelDev md;
};

int cu_count() {
    int n_cu = 256;
    { int dev = 0; hipGetDevice(&dev); hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev); if (n_cu < 1) n_cu = 256; }
    return n_cu;
}

// Set once a cooperative group has broken up in this process (a rank did not become resident within the wait limit: the device is
// shared with another process, or CUs are masked): from then on the library's OWN choice is plain chains -- every further call would
// pay the wait limit and the repeated solve again.  An explicit MOSHII_COOP_GROUP(g) / MOSHII_COOP=g request is still honoured.
static std::atomic<bool> g_coop_broke_once{false};   // (process-wide and sticky; solves may run on several host threads)
static void note_coop_broken(const char* where) {
    if (!g_coop_broke_once.exchange(true)) fprintf(stderr, "[moshii] %s: a cooperative group broke up (the device is shared?); the call is repeated with plain chains, "
                                            "and the library's own choice is plain chains for the rest of this process\n", where);
}
// test aid: MOSHII_COOP_SKEW=seed (read at every call) -> CoopDev::skew, the ranks' arrival order at the exchanges randomised
int coop_skew_env() {
    const char* e = getenv("MOSHII_COOP_SKEW");
    return (e && *e) ? atoi(e) : 0;
}
// The cooperative-chain request of a call: MOSHII_COOP_GROUP(g) in `flags` (0 = no word: the environment variable `env`, else the library's
// choice; 1 = plain chains; 2 .. 8 = that many workgroups per chain).  Returns -1 (library's choice), 0 (plain), g, or -2 (out of range).
int coop_request(uint32_t flags, const char* env) {
    int g = (int)((flags >> 8) & 0xffu);
    if (g == 0) {
        const char* e = getenv(env);
        if (!e) {
#ifdef MOSHII_EMULATION   // (the CPU emulation runs workgroups one after another unless told otherwise: a group would wait for itself)
            return 0;
#else
            return g_coop_broke_once.load() ? 0 : -1;
#endif
        }
        if (!strcmp(e, "auto")) return g_coop_broke_once.load() ? 0 : -1;   // (the library's choice, spelled out -- also how the emulation reaches it)
        g = atoi(e);
        if (g == 0) return 0;
    }
    if (g == 1) return 0;
    if (g < 0 || g > MOSHII_COOP_MAXG) return -2;
    return g;
}

// prepare_launch, part 1: validates the options; the sizes that follow from them
struct SolveDims { int xt, nshape, nmax, nblk, nkfmax, nhj, G, npose; };

int check_opts(moshii_model_t m, moshii_prior_t prior, const moshii_solve_opts* o, SolveDims* d) {
    if (!m->betas_set) return fail(MOSHII_ERR_ARG, "moshii_model_set_betas has not been called");
    if (o->n_body > 0 && (!prior || prior->npose != o->n_body)) return fail(MOSHII_ERR_ARG, "prior npose must equal n_body");
    if (o->n_step1 < 0 || o->n_step2 < 0 || o->n_step1 > m->NP || o->n_step2 > m->NP) return fail(MOSHII_ERR_ARG, "bad free-variable lists");
    const int NP = m->NP;
    const int nshape = o->n_shape;
    if (nshape < 0 || o->n_face < 0) return fail(MOSHII_ERR_ARG, "bad Step-2 extras");
    if (nshape > 0 && nshape != m->nshape) return fail(MOSHII_ERR_ARG, "n_shape must equal the block of moshii_model_set_free_shape");
    if (o->n_face > 0 && !o->face_ids) return fail(MOSHII_ERR_ARG, "face_ids missing");
    for (int i = 1; i < o->n_face; ++i)
        if (o->face_ids[i] != o->face_ids[i - 1] + 1) return fail(MOSHII_ERR_UNSUPPORTED, "face ids must be contiguous");
    if (o->n_jangle < 0 || (o->n_jangle > 0 && !o->jangle_ids)) return fail(MOSHII_ERR_ARG, "bad joint-angle term");
    for (int i = 0; i < o->n_jangle; ++i)
        if (o->jangle_ids[i] < 0 || o->jangle_ids[i] >= NP) return fail(MOSHII_ERR_ARG, "joint-angle id out of range");
    if (o->n_jangle > 0 && o->n_finger > 0)   // (the kernel sums the joint-angle term in the finger term's accumulator)
        return fail(MOSHII_ERR_UNSUPPORTED, "a joint-angle term and finger ids in one solve (no SMAL model has fingers)");
    const int xt = (nshape > 0 || o->n_face > 0) ? 1 : 0;
    const int nmax = 3 + std::max(o->n_step1, o->n_step2 + nshape);
    int nblk = pick_nblk(nmax, xt != 0);
    if (nblk < 0) return fail(MOSHII_ERR_UNSUPPORTED, xt ? "more than 207 unknowns per step" : "more than 124 free pose variables per step");
    if (const char* e = getenv("MOSHII_FORCE_NBLK")) nblk = std::max(nblk, atoi(e));
    auto count_kf = [&](const int32_t* ids, int n) {   // needed joints (superset over both steps)
        std::vector<char> need(m->K, 0);
        for (int i = 0; i < n; ++i) {
            if (ids[i] < 0 || ids[i] >= NP) return -1;
            if (ids[i] < m->body_dof) need[ids[i] / 3] = 1;
            else for (int k = m->body_dof / 3; k < m->K; ++k) need[k] = 1;
        }
        int c = 0; for (char b : need) c += b; return c;
    };
    const int kf1 = count_kf(o->step1_ids, o->n_step1), kf2 = count_kf(o->step2_ids, o->n_step2);
    if (kf1 < 0 || kf2 < 0) return fail(MOSHII_ERR_ARG, "free pose id out of range");
    if (o->n_finger > 0)
        for (int i = 1; i < o->n_finger; ++i)
            if (o->finger_ids[i] != o->finger_ids[i - 1] + 1) return fail(MOSHII_ERR_UNSUPPORTED, "finger ids must be contiguous");
    // hand joints whose d marker / d fullpose must be parked for the PCA contraction (only when hand coefficients are free)
    bool hand_free = false;
    for (int i = 0; i < o->n_step1; ++i) hand_free |= o->step1_ids[i] >= m->body_dof;
    for (int i = 0; i < o->n_step2; ++i) hand_free |= o->step2_ids[i] >= m->body_dof;
    d->xt = xt; d->nshape = nshape; d->nmax = nmax; d->nblk = nblk;
    d->nkfmax = std::max(1, std::max(kf1, kf2));
    d->nhj = hand_free ? (m->K - m->body_dof / 3) : 0;
    d->G = prior ? prior->G : 0; d->npose = prior ? prior->npose : 0;
    return MOSHII_OK;
}

// prepare_launch, part 2: the J^T J register tiling and the LDS layout -- marker-tile size Tm as large as the per-workgroup LDS
// budget allows; for cooperative chains one tile of a rank's largest possible share.
// coop_g: -1 = the library's choice, 0 = plain chains, 2 .. 8 = that many workgroups per chain.  The library chooses a group
// (solve_plan::own_group_size) when every workgroup of the launch can be resident at once (n_workgroups chains x g <= CUs).
int choose_layout(moshii_model_t m, const SolveDims& d, int Mmax, int Nvmax, int NWmax, int n_workgroups, int coop_g, LaunchCfg* cfg) {
    const int xt = d.xt, nmax = d.nmax, npose = d.npose;
    int nblk = d.nblk;
    auto layout = [&](int Tm) { return make_layout(m, Mmax, Nvmax, NWmax, npose, d.G, nmax, d.nkfmax, Tm, nblk, d.nhj, d.nshape); };
    // LDS budget per workgroup: the whole CU (160 KiB).  One workgroup per CU: a 256-register variant (two per CU) spilled and was
    // measured slower per chain by 1.9x for +6 % aggregate throughput (round 1, tools/gpu_occupancy.py); it was removed in round 3.
    const int n_cu = cu_count();
    int budget = 160 * 1024;
    if (const char* e = getenv("MOSHII_LDS_BUDGET")) budget = atoi(e);
    // Marker-tile size Tm (T0 maps tile vertices to threads 0..127: 3 Tm <= 120).  The Jacobian rows of a tile are built by
    // (tile marker, needed joint) items, 256 at a time, so among the sizes that fit the LDS budget take the one with the
    // fewest item rounds + tiles over a fully visible frame (53 markers x 20 joints: 38 + 15 = 3 + 2 rounds, where two equal
    // tiles of 27 / 26 cost 3 + 3), weighted by what a round and a tile's fixed work cost (about 3 : 4).
    int Tm;
    ChainLayout ly;
    if (coop_g == -1) coop_g = solve_plan::own_group_size(Mmax, d.nkfmax, npose > 0, !xt && nblk < 4);
    if (coop_g > 0 && ((!xt && nmax + 1 > 8 * 16) || (long long)coop_g * std::max(n_workgroups, 1) > n_cu)) coop_g = 0;   // (not built / not all resident: plain chains)
    if (coop_g > 0) {   // cooperative chains: a rank builds the rows of its own markers only -- one tile of its largest possible share
        if (!xt && nblk < 4) nblk = 4;   // (cooperative instantiations: 4, 5, 7, 8 register blocks; extended variant: 5, 8, 10, 13 as the plain one)
        if (nmax + 1 > nblk * 16) return fail(MOSHII_ERR_UNSUPPORTED, "cooperative chains: too many unknowns");
        if (coop_g > MOSHII_COOP_MAXG) return fail(MOSHII_ERR_ARG, "cooperative chains: at most 8 workgroups per chain");
        // with a prior: from three ranks on the last one does nothing but the prior (measured: its evaluation is as long as the others' forward pass)
        // (the extended variant's per-marker work -- shape columns, 13-block tiles -- outweighs the prior: its rank takes half a share of markers too;
        //  measured on config 3, eight ranks: 3.53 / 3.30 / 3.65 / 3.60 ms per cold frame at 0 / 0.5 / 0.8 / 1)
        cfg->coop_prior_frac = (npose > 0) ? ((coop_g >= 3) ? (xt ? 0.5 : 0.0) : 0.4) : 1.0;
        if (const char* e = getenv("MOSHII_COOP_PRIOR_FRAC")) cfg->coop_prior_frac = std::min(1.0, std::max(0.0, atof(e)));
        int mlo[MOSHII_COOP_MAXG + 1];
        coop_split(Mmax, coop_g, cfg->coop_prior_frac, mlo);
        int share = 2;
        for (int r = 0; r < coop_g; ++r) share = std::max(share, mlo[r + 1] - mlo[r]);
        Tm = std::min(40, share + 1);   // (+1: a chain with fewer markers than Mmax rounds its shares on its own)
        ly = layout(Tm);
        while (Tm > 2 && (size_t)ly.total_doubles * 8 > (size_t)budget) ly = layout(--Tm);   // (a share larger than the LDS leaves room for: several tiles per rank)
        cfg->coop = CoopLayout(nblk, Mmax, coop_g);
        cfg->coop_prior_rank = coop_g - 1;
    } else
    if (const char* e = getenv("MOSHII_TM")) {
        Tm = std::max(1, std::min(40, atoi(e)));
        ly = layout(Tm);
    } else {
        int best = -1, best_cost = 0;
        for (int t = std::min(40, std::max(2, Mmax)); t >= 2; --t) {
            const ChainLayout lt = layout(t);
            if ((size_t)lt.total_doubles * 8 > (size_t)budget) continue;
            const int full = Mmax / t, rem = Mmax % t;
            const int rounds = full * ((t * d.nkfmax + 255) / 256) + (rem ? (rem * d.nkfmax + 255) / 256 : 0);
            const int cost = 3 * rounds + 4 * (full + (rem ? 1 : 0));
            if (best < 0 || cost < best_cost) { best = t; best_cost = cost; }
        }
        if (best < 0) best = 2;   // (does not fit: reported below)
        Tm = best;
        ly = layout(Tm);
    }
    const size_t lds_bytes = (size_t)ly.total_doubles * sizeof(double);
    if (lds_bytes > 160 * 1024) return fail(MOSHII_ERR_UNSUPPORTED, "problem does not fit the 160 KiB LDS of a CU");
    cfg->nblk = nblk; cfg->xt = xt; cfg->ly = ly; cfg->lds_bytes = lds_bytes;
    cfg->coop_g = coop_g;
    return MOSHII_OK;
}

// prepare_launch, part 3: uploads the id lists to the head of the model's control scratch and fills the option / prior / model
// descriptors.  `extra_bytes` are reserved behind the id lists; their offset comes back through ctl_off.
int upload_ids(moshii_model_t m, moshii_prior_t prior, const moshii_solve_opts* o, hipStream_t stream, size_t extra_bytes, LaunchCfg* cfg,
               size_t* ctl_off) {
    const int nshape = o->n_shape, njangle = std::max(0, o->n_jangle);
    const size_t nids = (size_t)o->n_step1 + o->n_step2 + o->n_body + o->n_finger + o->n_face + njangle;
    const size_t need = sizeof(int) * (nids + 16) + 64 + extra_bytes;
    int rc = m->scratch.reserve(need, stream);
    if (rc) return rc;
    std::vector<int> ids;
    ids.reserve(nids);
    const size_t e1 = 0, e2 = e1 + o->n_step1, eb = e2 + o->n_step2, ef = eb + o->n_body;
    ids.insert(ids.end(), o->step1_ids, o->step1_ids + o->n_step1);
    ids.insert(ids.end(), o->step2_ids, o->step2_ids + o->n_step2);
    ids.insert(ids.end(), o->body_ids, o->body_ids + o->n_body);
    ids.insert(ids.end(), o->finger_ids, o->finger_ids + o->n_finger);
    const size_t efc = ids.size();
    ids.insert(ids.end(), o->face_ids, o->face_ids + o->n_face);
    const size_t eja = ids.size();
    if (njangle > 0) ids.insert(ids.end(), o->jangle_ids, o->jangle_ids + njangle);
    char* dbase = m->scratch.ptr;
    if (!ids.empty()) {
        HIP_TRY(hipMemcpyAsync(dbase, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // `ids` is pageable and goes out of scope
    }
    *ctl_off = (ids.size() * sizeof(int) + 63) & ~size_t(63);

    OptsDev& od = cfg->od;
    od.wt_data = o->wt_data; od.wt_velo = o->wt_velo; od.wt_poseB = o->wt_poseB; od.wt_poseH = o->wt_poseH;
    od.wt_annealing = o->wt_annealing; od.num_train_markers = o->num_train_markers;
    od.e3_first = o->e3_first; od.e3 = o->e3; od.delta0 = o->delta0; od.maxiter = o->maxiter;
    od.n1 = o->n_step1; od.n2 = o->n_step2; od.nbody = o->n_body; od.nfinger = o->n_finger;
    od.same_sets = (nshape == 0 && o->n_step1 == o->n_step2 && std::equal(o->step1_ids, o->step1_ids + o->n_step1, o->step2_ids)) ? 1 : 0;
    od.wt_poseF = o->wt_poseF; od.wt_shape = o->wt_shape; od.wt_shape_stay = o->wt_shape_stay;
    od.nface = o->n_face; od.nshape = nshape;
    const int* dids = (const int*)dbase;
    od.step1 = as_gp(dids + e1); od.step2 = as_gp(dids + e2); od.body = as_gp(dids + eb); od.finger = as_gp(dids + ef); od.face = as_gp(dids + efc);
    od.njangle = njangle; od.wt_jangle = njangle > 0 ? o->wt_jangle : 0.0; od.jangle = as_gp(dids + eja);
    memset(&cfg->pd, 0, sizeof(cfg->pd));
    if (prior) cfg->pd = prior->dev();
    cfg->md = m->dev();
    return MOSHII_OK;
}

int prepare_launch(moshii_model_t m, moshii_prior_t prior, const moshii_solve_opts* o, int Mmax, int Nvmax, int NWmax,
                   int n_workgroups, hipStream_t stream, size_t extra_bytes, LaunchCfg* cfg, size_t* ctl_off, int coop_g = 0) {
    SolveDims d;
    int rc;
    if ((rc = check_opts(m, prior, o, &d))) return rc;
    if ((rc = choose_layout(m, d, Mmax, Nvmax, NWmax, n_workgroups, coop_g, cfg))) return rc;
    // (the kernel body takes these distances for granted: a make_layout that no longer keeps them must not reach the device)
#ifdef MOSHII_EMULATION   // test hook of the CPU build only: the layout as a make_layout that had grown a field between dsd and dgn would leave it
    if (getenv("MOSHII_TEST_BREAK_LAYOUT")) { cfg->ly.o_dgn += 2; cfg->ly.o_ddl += 2; cfg->ly.o_y += 2; cfg->ly.o_red += 2; cfg->ly.o_scal += 2; }
#endif
    if (const char* why = chain_layout_fault(cfg->ly, cfg->nblk)) return fail(MOSHII_ERR_UNSUPPORTED, std::string("internal error: ") + why);
    return upload_ids(m, prior, o, stream, extra_bytes, cfg, ctl_off);
}

int launch_chains(const LaunchCfg& cfg, int n, const ChainDev* d_chains, hipStream_t stream) {
    HIP_TRY(moshii_launch_chain_solve(cfg.nblk, cfg.xt, n, cfg.lds_bytes, stream, d_chains, &cfg.md, &cfg.pd, &cfg.od, &cfg.ly, cfg.coop_g));
    note_launch("k_chain_solve<" + std::to_string(cfg.nblk) + ",1" + (cfg.xt ? ",xt" : "") +
                (cfg.coop_g > 0 ? ",coop" + std::to_string(cfg.coop_g) : "") + ">", (int)cfg.lds_bytes, MOSHII_TPB);
    return MOSHII_OK;
}

// extended variant: a chain's scratch for the shape derivatives of the joint transforms ([2][K][E][3] doubles) and, beyond 8 register
// blocks, the global packed factor + trash / zero words + a spare word per thread (ldl_big)
size_t qscratch_bytes(const LaunchCfg& cfg, int K, int E) {
    const size_t nfac = (cfg.nblk > 8) ? (size_t)(cfg.ly.nmax + 1) * (cfg.ly.nmax + 2) / 2 + 12 + 256 : 0;
    return ((size_t)2 * K * E * 3 + nfac) * sizeof(double);
}

// ---- cooperative chains: the exchange buffer kept with the model, laid out by cfg.coop --------------
int reserve_exchange(moshii_model_t m, const CoopLayout& cl, size_t n_chains, hipStream_t stream) {
    int rc = m->coopbuf.reserve(cl.bytes_per_chain * n_chains, stream);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(m->coopbuf.ptr, 0, cl.bytes_per_chain * n_chains, stream));   // flags and abort words start at zero on EVERY launch
    return MOSHII_OK;
}

void fill_coop(ChainDev& cd, const LaunchCfg& cfg, int M, char* slice) {   // slice: this chain's part of the exchange buffer
    cd.coop.G = cfg.coop_g; cd.coop.prior_rank = cfg.coop_prior_rank; cd.coop.slot_doubles = cfg.coop.slot_doubles; cd.coop.skew = coop_skew_env();
    coop_split(M, cfg.coop_g, cfg.coop_prior_frac, cd.coop.mlo);
    cd.coop.slots = as_gp_rw((unsigned long long*)slice);
    cd.coop.flags = as_gp_rw((unsigned*)(slice + cfg.coop.flags_offset));
}

// Did every group of the launch stay whole?  One strided copy of the chains' abort words (a copy per chain was 22 us a chain,
// 0.5-1 ms a round); synchronises the stream.
int coop_any_broken(moshii_model_t m, const CoopLayout& cl, size_t n_chains, hipStream_t stream, bool* broken) {
    std::vector<unsigned> ab(n_chains, 0u);
    HIP_TRY(hipMemcpy2DAsync(ab.data(), sizeof(unsigned), m->coopbuf.ptr + cl.abort_offset, cl.bytes_per_chain, sizeof(unsigned), n_chains,
                             hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *broken = false;
    for (unsigned a : ab) *broken |= a != 0u;
    return MOSHII_OK;
}

// ---- the device buffers a call allocates for itself (MOSHII_BUFFERS_HOST callers; a start state) ----
struct FrameBufs {   // the per-frame arrays shared by moshii_chain_desc and moshii_sequence_desc
    int F, M;
    const double* obs; const uint8_t* vis;
    double *pose, *fullpose, *trans, *msim, *errs; int *iters, *status;
    double* shape;   // extended variant: the rows of free shape coefficients (or null)
};
struct Staged {   // device copies of one chain's / sequence's per-frame host buffers: freed on every way out
    FrameBufs rows = {};
    DevArena mem;   // owns what `rows` points to
};
struct CallBufs {
    std::vector<Staged> st;      // per chain / sequence; empty for MOSHII_BUFFERS_DEVICE callers
    DevArena mem;                // moshii_sequence_solve: start states of the sequences that continue a chain
    explicit CallBufs(size_t n) : st(n) {}
};

// device copies of the inputs of `h`, zeroed rows for its outputs (n_shape > 0: and that many shape coefficients)
int stage_in(const FrameBufs& h, int NP, int P, size_t n_shape, hipStream_t stream, Staged* s) {
    const size_t Fz = std::max(h.F, 1), M = h.M;
    FrameBufs& d = s->rows;
    d.F = h.F; d.M = h.M;
    DevArena& mem = s->mem;
    d.obs = mem.upload(h.obs, (size_t)h.F * M * 3);
    d.vis = mem.upload(h.vis, (size_t)h.F * M);
    d.pose = mem.zeros<double>(Fz * NP, stream);
    d.fullpose = mem.zeros<double>(Fz * P, stream);
    d.trans = mem.zeros<double>(Fz * 3, stream);
    d.msim = mem.zeros<double>(Fz * M * 3, stream);
    d.errs = mem.zeros<double>(Fz * MOSHII_NERR, stream);
    d.iters = mem.zeros<int>(Fz * 2, stream);
    d.status = mem.zeros<int>(Fz, stream);
    if (n_shape > 0) d.shape = mem.zeros<double>(n_shape, stream);
    return mem.ok() ? MOSHII_OK : fail_mem(mem, "staging a chain's frames");
}

// copies the results back (the stream has been synchronised); `s` frees the device copies when it goes
int stage_out(const FrameBufs& h, int NP, int P, int E, const Staged& s) {
    const size_t F = h.F, M = h.M;
    const FrameBufs& d = s.rows;
    if (!F) return MOSHII_OK;
    if (h.pose) HIP_TRY(hipMemcpy(h.pose, d.pose, F * NP * sizeof(double), hipMemcpyDeviceToHost));
    if (h.fullpose) HIP_TRY(hipMemcpy(h.fullpose, d.fullpose, F * P * sizeof(double), hipMemcpyDeviceToHost));
    if (h.trans) HIP_TRY(hipMemcpy(h.trans, d.trans, F * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (h.msim) HIP_TRY(hipMemcpy(h.msim, d.msim, F * M * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (h.errs) HIP_TRY(hipMemcpy(h.errs, d.errs, F * MOSHII_NERR * sizeof(double), hipMemcpyDeviceToHost));
    if (h.iters) HIP_TRY(hipMemcpy(h.iters, d.iters, F * 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (h.status) HIP_TRY(hipMemcpy(h.status, d.status, F * sizeof(int), hipMemcpyDeviceToHost));
    if (h.shape && d.shape) HIP_TRY(hipMemcpy(h.shape, d.shape, F * E * sizeof(double), hipMemcpyDeviceToHost));
    return MOSHII_OK;
}

// max |entry_c - final_pred(c)| per chunk (pose, trans, and pose_prev when the velocity term is live), or one of the verdicts
// MOSHII_HANDOFF_* (solve_plan.h) where the states cannot be compared.
__global__ void k_verify_chunks(int n, int NP, int E, const int* __restrict__ pred, const double* __restrict__ entry,
                                const double* __restrict__ fin, double* __restrict__ dev) {
    const int c = blockIdx.x;
    if (c >= n) return;
    const int p = pred[c];
    __shared__ double red[64];
    double d = 0.0;
    if (p >= 0) {
        const int S = 2 * NP + 5 + E;
        const double* a = entry + (size_t)c * S;
        const double* b = fin + (size_t)p * S;
        const bool flags_ok = (a[2 * NP + 3] == b[2 * NP + 3]) && (a[2 * NP + 4] == b[2 * NP + 4]);
        const bool hp = a[2 * NP + 3] != 0.0;
        bool nan = false;   // (fmax drops a NaN operand: track it separately, a NaN hand-off must never pass as deviation 0)
        for (int i = threadIdx.x; i < 2 * NP + 3; i += blockDim.x) {
            if (i >= NP && i < 2 * NP && !hp) continue;
            const double v = fabs(a[i] - b[i]);
            nan |= !(v == v);
            d = fmax(d, v);
        }
        for (int e = threadIdx.x; e < E; e += blockDim.x) {   // free shape block
            const double v = fabs(a[2 * NP + 5 + e] - b[2 * NP + 5 + e]);
            nan |= !(v == v);
            d = fmax(d, v);
        }
        if (nan) d = MOSHII_HANDOFF_NAN;
        else if (a[2 * NP + 3] == MOSHII_MARK_ENTRY_SPOILED && b[2 * NP + 3] != MOSHII_MARK_FINAL_SPOILED) d = MOSHII_HANDOFF_GIVEN_UP;
        else if (b[2 * NP + 3] == MOSHII_MARK_FINAL_SPOILED) d = MOSHII_HANDOFF_PRED_GIVEN_UP;
        else if (!flags_ok) d = MOSHII_HANDOFF_MISMATCH;
    }
    red[threadIdx.x] = d;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) dev[c] = red[0];
}

// ---- moshii_chain_solve ------------------------------------------------------------------------------
// One launch of the chains.  *broken: a cooperative group broke up -- a workgroup of it did not show up within the wait limit (the chip
// is shared with another process?) -- and the caller repeats the solve with plain chains.
int chain_solve_once(moshii_model_t m, moshii_prior_t prior, const moshii_solve_opts* o, int32_t n_chains, const moshii_chain_desc* chains,
                     uint32_t flags, hipStream_t stream, bool* broken) {
    *broken = false;
    const bool dev = (flags & MOSHII_BUFFERS_DEVICE) != 0;
    const int NP = m->NP, P = m->P;
    int Mmax = 0, Nvmax = 0, NWmax = 1;
    for (int c = 0; c < n_chains; ++c) {
        const moshii_chain_desc& ch = chains[c];
        if (!ch.attach || ch.attach->model != m || ch.F < 0 || !ch.obs || !ch.vis) return fail(MOSHII_ERR_ARG, "bad chain descriptor");
        Mmax = std::max(Mmax, ch.attach->M); Nvmax = std::max(Nvmax, ch.attach->Nv); NWmax = std::max(NWmax, ch.attach->NW);
    }
    // control block after the id lists: [ChainDev x n][init vectors]
    const int E = o->n_shape > 0 ? o->n_shape : 0;
    const size_t extra = sizeof(ChainDev) * n_chains + sizeof(double) * (size_t)n_chains * (2 * NP + 4 + E + 2) + 256;
    // cooperative chains (MOSHII_COOP_GROUP(g) in `flags`, or MOSHII_COOP=g): g workgroups per chain, all of them resident at once
    int coop_req = coop_request(flags, "MOSHII_COOP");
    if (coop_req < -1) return fail(MOSHII_ERR_ARG, "cooperative chains: group size out of range");
    LaunchCfg cfg;
    size_t ctl = 0;
    int rc = prepare_launch(m, prior, o, Mmax, Nvmax, NWmax, n_chains, stream, extra, &cfg, &ctl, coop_req);
    if (rc) return rc;
    const int coop_g = cfg.coop_g;   // (0: plain chains -- asked for, or the group does not fit the chip / the solve is an extended one)
    if (coop_g > 0 && (rc = reserve_exchange(m, cfg.coop, n_chains, stream))) return rc;
    char* dbase = m->scratch.ptr + ctl;
    const size_t qbytes = qscratch_bytes(cfg, m->K, E);
    const int qranks = (coop_g > 0) ? coop_g : 1;   // (cooperative chains: a slice per rank -- every rank keeps its own derivative arrays / factor)
    if (E > 0 && (rc = m->qscratch.reserve(qbytes * n_chains * qranks, stream))) return rc;
    std::vector<char> hostbuf(extra, 0);
    size_t off = sizeof(ChainDev) * n_chains;
    auto put = [&](const void* src, size_t bytes) { off = (off + 15) & ~size_t(15); size_t o2 = off; memcpy(hostbuf.data() + off, src, bytes); off += bytes; return o2; };
    CallBufs bufs(dev ? 0 : n_chains);
    std::vector<FrameBufs> fbs(n_chains);
    std::vector<ChainDev> cds(n_chains);
    for (int c = 0; c < n_chains; ++c) {
        const moshii_chain_desc& ch = chains[c];
        ChainDev& cd = cds[c];
        memset(&cd, 0, sizeof(cd));
        cd.att = ch.attach->d_self; cd.F = ch.F; cd.first = ch.first_frame_schedule;
        if (coop_g > 0) fill_coop(cd, cfg, ch.attach->M, m->coopbuf.ptr + cfg.coop.bytes_per_chain * c);
        if (ch.init_pose) cd.init_pose = (const double*)(dbase + put(ch.init_pose, sizeof(double) * NP));
        if (ch.init_trans) cd.init_trans = (const double*)(dbase + put(ch.init_trans, sizeof(double) * 3));
        if (ch.init_pose_prev) cd.init_prev = (const double*)(dbase + put(ch.init_pose_prev, sizeof(double) * NP));
        if (E > 0) {
            if (ch.init_shape) cd.init_shape = (const double*)(dbase + put(ch.init_shape, sizeof(double) * E));
            cd.qscratch = (double*)(m->qscratch.ptr + qbytes * (size_t)c * qranks);
            cd.coop.qstride = (int)(qbytes / sizeof(double));
        }
        fbs[c] = FrameBufs{ch.F, ch.attach->M, ch.obs, ch.vis, ch.pose, ch.fullpose, ch.trans, ch.markers_sim, ch.errs, ch.iters, ch.status, E > 0 ? ch.shape : nullptr};
        if (!dev && (rc = stage_in(fbs[c], NP, P, (fbs[c].shape && ch.F > 0) ? (size_t)ch.F * E : 0, stream, &bufs.st[c]))) return rc;
        const FrameBufs& b = dev ? fbs[c] : bufs.st[c].rows;   // where the chain finds its rows
        cd.obs = b.obs; cd.vis = b.vis; cd.pose = b.pose; cd.fullpose = b.fullpose; cd.trans = b.trans;
        cd.msim = b.msim; cd.errs = b.errs; cd.iters = b.iters; cd.status = b.status; cd.shape = b.shape;
    }
    if (off > extra) return fail(MOSHII_ERR_ARG, "internal: scratch overflow");
    memcpy(hostbuf.data(), cds.data(), sizeof(ChainDev) * n_chains);
    HIP_TRY(hipMemcpyAsync(dbase, hostbuf.data(), off, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // hostbuf is pageable and goes out of scope
    if ((rc = launch_chains(cfg, n_chains, (const ChainDev*)dbase, stream))) return rc;
    // (the call synchronises: a broken group has to be reported, not left in the rows)
    if (coop_g > 0) {
        if ((rc = coop_any_broken(m, cfg.coop, n_chains, stream, broken))) return rc;
        if (*broken) return MOSHII_OK;
    }
    if (!dev) {
        HIP_TRY(hipStreamSynchronize(stream));
        for (int c = 0; c < n_chains; ++c)
            if ((rc = stage_out(fbs[c], NP, P, E, bufs.st[c]))) return rc;
    }
    return MOSHII_OK;
}

// ---- moshii_sequence_solve, step by step: plan, prepare, stage, launch_pass1, { verify, solve_plan::pick_repairs, repair_round }, finish ----
struct SeqSolve {
    const moshii_model_t m; const moshii_prior_t prior; const moshii_solve_opts* const o;
    const int n_seq; const moshii_sequence_desc* const seqs; const moshii_chunk_opts* const co; const uint32_t flags; const hipStream_t stream;
    const bool dev = (flags & MOSHII_BUFFERS_DEVICE) != 0;
    const int NP = m->NP, P = m->P, E = o->n_shape, S = 2 * NP + 5 + E;   // hand-off state: [pose][pose_prev][trans][has_prev][first][shape]
    const int warmup = co ? std::max(0, co->warmup) : 32;
    const double tol = (co && co->verify_tol > 0.0) ? co->verify_tol : 1e-11;
    const bool rejoin = getenv("MOSHII_NO_REJOIN") == nullptr;   // repair chains stop where they re-join the stored trajectory
    int Mmax = 0, Nvmax = 0, NWmax = 1, n_cu = 256, NC = 0;
    std::vector<Chunk> chunks;
    LaunchCfg cfg;
    size_t ctl = 0, extra = 0;   // the control block behind the id lists (prepare)
    ChainDev *d_pass1 = nullptr, *d_repair = nullptr;
    int *d_pred = nullptr, *d_bnd = nullptr, *d_done = nullptr, *d_baton = nullptr, *d_abort_at = nullptr, *d_fuse = nullptr, *d_fuse_count = nullptr;
    double *d_entry = nullptr, *d_final = nullptr, *d_dev = nullptr;   // hand-off states [NC][S] x 2 and deviations [NC]
    int coop_rep = 0;            // workgroups per repair chain (0: plain chains)
    bool fuse = false, trace = false;
    std::vector<LaunchCfg> coop_cfgs = std::vector<LaunchCfg>(MOSHII_COOP_MAXG + 1);   // per group size, prepared when first used (coop_g set)
    CallBufs bufs{dev ? (size_t)0 : (size_t)n_seq};   // the device buffers of this call: released on EVERY way out of it
    const double* d_init = nullptr;                   // start states of the sequences that continue a chain (in bufs.mem)
    std::vector<FrameBufs> fbs, dbs;                  // the caller's rows; where the chains find them on the device
    size_t qbytes = 0;
    std::vector<double> hdev;    // the last verification's hand-off deviations / verdicts
    int n_repaired = 0, rounds = 0;

    int plan() {
        std::vector<int> frames(n_seq);
        for (int q = 0; q < n_seq; ++q) {
            const moshii_sequence_desc& sq = seqs[q];
            if (!sq.attach || sq.attach->model != m || sq.F < 0 || !sq.obs || !sq.vis) return fail(MOSHII_ERR_ARG, "bad sequence descriptor");
            Mmax = std::max(Mmax, sq.attach->M); Nvmax = std::max(Nvmax, sq.attach->Nv); NWmax = std::max(NWmax, sq.attach->NW);
            frames[q] = sq.F;
        }
        n_cu = cu_count();
        chunks = solve_plan::chunk_table(frames, co ? co->num_chunks : 0, warmup, n_cu);   // (num_chunks: chunks per sequence when > 0)
        NC = (int)chunks.size();
        return MOSHII_OK;
    }

    // The launch configuration, the control block [ChainDev x NC (pass 1)][ChainDev x NC (repairs)][control words x 10 NC + 1], how the
    // repairs run (carried on inside the first launch / plain rounds / cooperative rounds) and the buffers kept with the model.
    int prepare() {
        extra = 2 * sizeof(ChainDev) * NC + 10 * sizeof(int) * NC + 256;
        int rc = prepare_launch(m, prior, o, Mmax, Nvmax, NWmax, NC, stream, extra, &cfg, &ctl);
        if (rc) return rc;
        d_pass1 = (ChainDev*)(m->scratch.ptr + ctl);
        d_repair = d_pass1 + NC;
        d_pred = (int*)(d_repair + NC);
        d_bnd = d_pred + NC;   // first frame of every chunk (the boundaries a run-through repair chain crosses)
        d_done = d_bnd + NC;   // frames processed per repair chain (diagnostics)
        d_baton = d_done + NC; // [2 NC] state / stop request per chunk (ChainDev::baton)
        d_abort_at = d_baton + 2 * NC;   // [NC] ChainDev::abort_at (kept across the rounds of this call)
        d_fuse = d_abort_at + NC;        // [3 NC] ChainDev::fuse_flags, then [1] ChainDev::fuse_count
        d_fuse_count = d_fuse + 3 * NC;
        // Pass-1 chains check their own right-hand hand-off and carry on as the repair chain of the next chunk when it misses
        // (ChainDev::fuse_F): possible when every chunk has a CU of its own for the whole launch, so that the flags they wait on are set.
        // Cooperative repair chains (MOSHII_COOP_GROUP(g) in `flags`, or MOSHII_COOP_REPAIR=g): the sweeps that bound a chunked solve run with g
        // workgroups each (csrc/moshii_dev.h: CoopDev), launched by the host's rounds -- a pass-1 chain cannot recruit CUs, so with them the
        // chains do not carry on inside the first launch.
        coop_rep = coop_request(flags, "MOSHII_COOP_REPAIR");
        if (coop_rep < -1) return fail(MOSHII_ERR_ARG, "cooperative chains: group size out of range");
        if (coop_rep == -1)   // the library's choice: as moshii_chain_solve picks it for one chain (choose_layout)
            coop_rep = solve_plan::own_group_size(Mmax, cfg.ly.nkfmax, prior && o->n_body > 0, cfg.ly.nmax + 1 > 8 * 16 || cfg.nblk < 4);
        if (coop_rep < 2 || E > 0 || o->n_face > 0 || !rejoin) coop_rep = 0;
        fuse = rejoin && NC <= n_cu && getenv("MOSHII_NO_FUSE") == nullptr && coop_rep == 0;
        trace = getenv("MOSHII_TRACE_REPAIR") != nullptr;
        if (coop_rep >= 2) {
            // the exchange buffers of the repair rounds, once and for the largest round this call can launch (a buffer that grows from
            // round to round is a hipFree + hipMalloc in the middle of the solve)
            const CoopLayout largest(std::max(4, cfg.nblk), Mmax, coop_rep);
            if ((rc = m->coopbuf.reserve(largest.bytes_per_chain * (size_t)std::min(NC, std::max(1, n_cu / 2))))) return rc;
        }
        // (kept with the model between calls: three hipMalloc / hipFree pairs a call were ~0.3 ms of a 37 ms step)
        if ((rc = m->handoff.reserve(((size_t)2 * NC * S + NC) * sizeof(double), stream))) return rc;
        d_entry = (double*)m->handoff.ptr;
        d_final = d_entry + (size_t)NC * S;
        d_dev = d_final + (size_t)NC * S;
        return MOSHII_OK;
    }

    int stage() {
        int rc;
        // start states of sequences that continue a chain (moshii_sequence_desc.init_*): [pose][pose_prev][trans][has_prev][first = 0]
        bool any = false;
        for (int q = 0; q < n_seq; ++q) any |= seqs[q].init_pose != nullptr;
        if (any) {
            std::vector<double> hinit((size_t)n_seq * S, 0.0);
            for (int q = 0; q < n_seq; ++q) {
                const moshii_sequence_desc& sq = seqs[q];
                if (!sq.init_pose) continue;
                if (!sq.init_trans) return fail(MOSHII_ERR_ARG, "init_trans is required with init_pose");
                double* h = hinit.data() + (size_t)q * S;
                memcpy(h, sq.init_pose, sizeof(double) * NP);
                if (sq.init_pose_prev) memcpy(h + NP, sq.init_pose_prev, sizeof(double) * NP);
                memcpy(h + 2 * NP, sq.init_trans, sizeof(double) * 3);
                h[2 * NP + 3] = sq.init_pose_prev ? 1.0 : 0.0;
                h[2 * NP + 4] = 0.0;
                if (E > 0 && sq.init_shape) memcpy(h + 2 * NP + 5, sq.init_shape, sizeof(double) * E);
            }
            d_init = bufs.mem.upload(hinit.data(), hinit.size());
            if (!bufs.mem.ok()) return fail_mem(bufs.mem, "moshii_sequence_solve: start states");
        }
        fbs.resize(n_seq); dbs.resize(n_seq);
        for (int q = 0; q < n_seq; ++q) {
            const moshii_sequence_desc& sq = seqs[q];
            fbs[q] = FrameBufs{sq.F, sq.attach->M, sq.obs, sq.vis, sq.pose, sq.fullpose, sq.trans, sq.markers_sim, sq.errs, sq.iters, sq.status, E > 0 ? sq.shape : nullptr};
            if (!dev && (rc = stage_in(fbs[q], NP, P, (E > 0 && sq.F >= 1) ? (size_t)sq.F * E : 0, stream, &bufs.st[q]))) return rc;
            dbs[q] = dev ? fbs[q] : bufs.st[q].rows;
        }
        if (E > 0) {   // extended variant: per-chain scratch for the shape derivatives of the joint transforms
            qbytes = qscratch_bytes(cfg, m->K, E);
            if ((rc = m->qscratch.reserve(qbytes * NC, stream))) return rc;
        }
        return MOSHII_OK;
    }

    // a chain over frames [from, ck.e) of its sequence; rows are addressed relative to `from`
    ChainDev make_chain(const Chunk& ck, int from, int idx, bool repair) const {
        const FrameBufs& b = dbs[ck.seq];
        const size_t M = b.M;
        ChainDev cd;
        memset(&cd, 0, sizeof(cd));
        cd.att = seqs[ck.seq].attach->d_self;
        cd.F = ck.e - from; cd.first = 1; cd.skip = ck.s - from;
        cd.obs = b.obs + (size_t)from * M * 3; cd.vis = b.vis + (size_t)from * M;
        cd.pose = b.pose ? b.pose + (size_t)from * NP : nullptr;
        cd.fullpose = b.fullpose ? b.fullpose + (size_t)from * P : nullptr;
        cd.trans = b.trans ? b.trans + (size_t)from * 3 : nullptr;
        cd.msim = b.msim ? b.msim + (size_t)from * M * 3 : nullptr;
        cd.errs = b.errs ? b.errs + (size_t)from * MOSHII_NERR : nullptr;
        cd.iters = b.iters ? b.iters + (size_t)from * 2 : nullptr;
        cd.status = b.status ? b.status + (size_t)from : nullptr;
        if (E > 0) {
            cd.shape = b.shape ? b.shape + (size_t)from * E : nullptr;
            cd.qscratch = (double*)(m->qscratch.ptr + qbytes * idx);      // repair chains reuse the slot of their first chunk
        }
        cd.final_state = d_final + (size_t)idx * S;
        // every chain records the state with which it enters its first recorded frame; a repair chain's is the
        // predecessor's end state it was started from, so if that predecessor is itself re-solved later the
        // mismatch shows up in the next verification and this chunk is repaired again
        cd.entry_state = d_entry + (size_t)idx * S;
        if (repair) {
            cd.init_state = d_final + (size_t)ck.pred * S;
            cd.rejoin_tol = rejoin ? tol : 0.0;
        } else if (ck.pred < 0 && d_init != nullptr && seqs[ck.seq].init_pose != nullptr) {
            cd.init_state = d_init + (size_t)ck.seq * S;   // the sequence continues a chain instead of starting one
        }
        return cd;
    }

    // ... which, its frame 0 being frame `from` of the sequence, re-solves chunk c0 and runs on through the following chunks to the end of the sequence
    void run_through(ChainDev& cd, int c0, int from) const {
        int cl = c0 + 1;   // one past the last chunk this chain may cover: the end of its sequence
        while (cl < NC && chunks[cl].seq == chunks[c0].seq) ++cl;
        cd.F = chunks[cl - 1].e - from;
        cd.final_state = d_final + (size_t)(cl - 1) * S;
        cd.nb = cl - 1 - c0;
        cd.bnd = d_bnd + c0 + 1;
        cd.bnd_off = from;
        cd.run_final = d_final + (size_t)c0 * S;
        cd.run_entry = d_entry + (size_t)c0 * S;
        cd.baton = d_baton;
        cd.abort_at = d_abort_at;
        cd.chunk0 = c0;
    }

    // The tail of pass 1 (ChainDev::tail_done): with cooperative repair sweeps the first launch's chains do not carry on, so the launch lasts as
    // long as its slowest chunk while the CUs of the others idle.  Once all but a fifth of a chip's worth of chains have ended, a chain with
    // more than a few frames to go gives its chunk up to the sweeps (which re-solve 16 frames in 2.5 ms).  MOSHII_TAIL_CUT=0 switches it off.
    void arm_tail_cut(std::vector<ChainDev>& cds) const {
        static const int tail_env = []{ const char* e = getenv("MOSHII_TAIL_CUT"); return e ? atoi(e) : -1; }();
        const int spare = tail_env > 0 ? tail_env : std::max(8, n_cu / 5);     // (a tenth of the chip: 65.4 k frames/s on the bench's six sequences; a fifth: 65.9 k; none: 63.4 k)
        // Only where it pays: every chunk on a CU of its own from the start (one wave of workgroups: the order of finishing is the order of
        // speed -- with 2 048 chunks the last to finish are simply the last to have started: measured 867 -> 617 k frames/s on the
        // 256-sequence job when armed there) and chunks so short that re-solving one costs less than the wait it ends (a 16-frame chunk:
        // 2.5 ms of a cooperative sweep; the 195-frame chunks of a 50 000-frame sequence: 30 ms -- 372 -> 226 k frames/s when armed).
        int longest = 0;
        for (int c = 0; c < NC; ++c) longest = std::max(longest, chunks[c].e - chunks[c].s);
        if (!(!fuse && coop_rep >= 2 && rejoin && tail_env != 0 && NC >= 4 * spare && NC <= n_cu && longest <= 32)) return;
        for (int c = 0; c < NC; ++c) {
            ChainDev& cd = cds[c];
            cd.tail_done = d_fuse_count;                // (the carry-on counter: unused without the carry-on protocol, zeroed with the control words)
            cd.tail_quota = NC - spare;
            cd.tail_left = 3;
            cd.tail_can_cut = chunks[c].pred >= 0 ? 1 : 0;
            cd.tail_mark = d_abort_at + c;
        }
    }

    // The pass-1 descriptors (plain; carrying on; giving up in the launch's tail) and the control words, then the first launch.
    int launch_pass1() {
        std::vector<ChainDev> cds(NC);
        for (int c = 0; c < NC; ++c) cds[c] = make_chain(chunks[c], chunks[c].a, c, false);
        if (fuse)
            for (int c = 0; c < NC; ++c) {
                ChainDev& cd = cds[c];
                cd.fuse_flags = d_fuse; cd.fuse_c = c; cd.fuse_count = d_fuse_count; cd.fuse_tol = tol;
                cd.fuse_has_prev = (chunks[c].pred >= 0) ? 1 : 0;
                const bool has_next = c + 1 < NC && chunks[c + 1].seq == chunks[c].seq;
                if (!has_next) continue;
                // its own chunk as before, then -- if the hand-off to chunk c + 1 misses -- the repair chain that starts at chunk c + 1
                cd.fuse_F = chunks[c].e - chunks[c].a;
                cd.fuse_has_next = 1;
                run_through(cd, c + 1, chunks[c].a);
                cd.rejoin_tol = tol;
            }
        arm_tail_cut(cds);
        HIP_TRY(hipMemcpyAsync(d_pass1, cds.data(), sizeof(ChainDev) * NC, hipMemcpyHostToDevice, stream));
        {   // the control words behind the descriptors in ONE copy: [pred][chunk starts][done][baton x 2 = 0][abort_at = -1: no mark][fuse flags x 3, fuse count = 0]
            std::vector<int> words((size_t)10 * NC + 1, 0);
            for (int c = 0; c < NC; ++c) { words[c] = chunks[c].pred; words[(size_t)NC + c] = chunks[c].s; words[(size_t)5 * NC + c] = -1; }
            HIP_TRY(hipMemcpyAsync(d_pred, words.data(), sizeof(int) * words.size(), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));   // (`words` goes out of scope)
        }
        int rc = launch_chains(cfg, NC, d_pass1, stream);
        if (rc) return rc;
        hdev.assign(NC, 0.0);
        if (fuse) {   // chains that carried on inside the first launch count as repairs (they did a repair chain's work)
            HIP_TRY(hipMemcpyAsync(&n_repaired, d_fuse_count, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (trace) fprintf(stderr, "[moshii] pass 1: %d chains carried on into the next chunk\n", n_repaired);
        }
        return MOSHII_OK;
    }

    // hdev[c]: how far chunk c's entry state is from its predecessor's end state, or a verdict (k_verify_chunks)
    int verify() {
        hipLaunchKernelGGL(k_verify_chunks, dim3(NC), dim3(64), 0, stream, NC, NP, E, d_pred, d_entry, d_final, d_dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hdev.data(), d_dev, sizeof(double) * NC, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (rounds == 0) if (const char* dump = getenv("MOSHII_DUMP_HANDOFF")) {   // diagnostics: first-pass hand-off deviations
            if (FILE* fp = fopen(dump, "w")) {
                for (int c = 0; c < NC; ++c) fprintf(fp, "%d %d %d %d %.6e\n", chunks[c].seq, chunks[c].a, chunks[c].s, chunks[c].e, hdev[c]);
                fclose(fp);
            }
        }
        if (trace && NC <= 16) { fprintf(stderr, "[moshii] hand-off deviations:"); for (int c = 0; c < NC; ++c) fprintf(stderr, " %.1e", hdev[c]); fprintf(stderr, "\n"); }
        return MOSHII_OK;
    }

    // a round of cooperative sweeps, g_round workgroups each: its launch configuration (prepared when first used) and exchange buffers
    int prepare_coop_round(int g_round, const std::vector<int>& todo, std::vector<ChainDev>& rep) {
        int rc;
        LaunchCfg& cc = coop_cfgs[g_round];
        if (cc.coop_g != g_round) {
            size_t ctl2 = 0;
            // (n_workgroups = 1: the residency of this round's chains has been settled by the caller)
            if ((rc = prepare_launch(m, prior, o, Mmax, Nvmax, NWmax, 1, stream, extra, &cc, &ctl2, g_round))) return rc;
            if (cc.coop_g != g_round) return fail(MOSHII_ERR_ARG, "internal: cooperative repair launch not prepared");
            if (ctl2 != ctl) return fail(MOSHII_ERR_ARG, "internal: control block moved");
        }
        if ((rc = reserve_exchange(m, cc.coop, rep.size(), stream))) return rc;
        for (size_t i = 0; i < rep.size(); ++i)
            fill_coop(rep[i], cc, seqs[chunks[todo[i]].seq].attach->M, m->coopbuf.ptr + cc.coop.bytes_per_chain * i);
        return MOSHII_OK;
    }

    // Re-solves (exactly, from the predecessor's final state) the chunks of `todo` in one launch.
    // Every repair chain starts at its failing chunk and runs on through the following chunks of its sequence until it
    // re-joins the stored trajectory.  Where it reaches the start of another chain of this round, it takes over from it
    // (ChainDev::baton): a cascade of adjacent wrong regions is swept by ONE chain in one round, while regions that turn
    // out to be independent are still repaired side by side.  (Before the baton each chain ended at the next chain's
    // start: a cascade cost one round per region, each as long as the longest chain of that round.)
    int repair_round(const std::vector<int>& todo) {
        int rc;
        std::vector<ChainDev> rep(todo.size());
        std::vector<int> hbaton(2 * (size_t)NC, 0);
        for (size_t i = 0; i < todo.size(); ++i) {
            const int c = todo[i];
            hbaton[2 * (size_t)c] = 1;
            ChainDev& cd = rep[i] = make_chain(chunks[c], chunks[c].s, c, true);
            run_through(cd, c, chunks[c].s);
            if (!rejoin) { cd.F = chunks[c].e - chunks[c].s; cd.nb = 0; cd.final_state = d_final + (size_t)c * S; cd.baton = nullptr; cd.abort_at = nullptr; }   // (one chunk per chain)
            cd.frames_done = trace ? d_done + i : nullptr;
        }
        // cooperative sweeps: as many workgroups per chain as the request and the chip allow (every workgroup of the launch resident)
        const int g_round = (coop_rep >= 2) ? std::min(coop_rep, n_cu / (int)rep.size()) : 0;
        if (g_round >= 2 && (rc = prepare_coop_round(g_round, todo, rep))) return rc;
        const LaunchCfg& use = (g_round >= 2) ? coop_cfgs[g_round] : cfg;
        HIP_TRY(hipMemcpyAsync(d_baton, hbaton.data(), sizeof(int) * hbaton.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_repair, rep.data(), sizeof(ChainDev) * rep.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if ((rc = launch_chains(use, (int)rep.size(), d_repair, stream))) return rc;
        if (g_round >= 2) {
            bool broken = false;
            if ((rc = coop_any_broken(m, use.coop, rep.size(), stream, &broken))) return rc;
            if (broken) {   // (the chip is shared?)  Whatever the broken groups left is caught by the next verification -- they spoil the entry state of
                            // the chunk they stopped in -- and re-solved by plain chains from here on
                note_coop_broken("moshii_sequence_solve");
                coop_rep = 0;
            }
        }
        n_repaired += (int)rep.size();
        ++rounds;
        if (trace) {
            std::vector<int> done(rep.size(), -1);
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipMemcpy(done.data(), d_done, sizeof(int) * rep.size(), hipMemcpyDeviceToHost));
            fprintf(stderr, "[moshii] repair round %d: %zu chains (chunk:dev:frames_done/limit)", rounds, rep.size());
            for (size_t i = 0; i < rep.size(); ++i) fprintf(stderr, " %d:%.0e:%d/%d", todo[i], hdev[todo[i]], done[i], rep[i].F);
            fprintf(stderr, "\n");
        }
        return MOSHII_OK;
    }

    int finish(moshii_chunk_report* report) {
        double max_dev = 0.0;
        for (int c = 0; c < NC; ++c) if (chunks[c].pred >= 0) max_dev = std::max(max_dev, hdev[c]);
        if (report) { report->n_chunks = NC; report->n_repaired = n_repaired; report->repair_rounds = rounds; report->max_handoff_dev = max_dev;
                      report->warmup = warmup; report->verify_tol = tol; }
        if (dev) return MOSHII_OK;
        int rc;
        HIP_TRY(hipStreamSynchronize(stream));
        for (int q = 0; q < n_seq; ++q)
            if ((rc = stage_out(fbs[q], NP, P, E, bufs.st[q]))) return rc;
        return MOSHII_OK;
    }
};

}  // namespace

extern "C" {

int moshii_chain_solve(moshii_model_t m, moshii_prior_t prior, const moshii_solve_opts* o, int32_t n_chains,
                       const moshii_chain_desc* chains, uint32_t flags, void* stream_) {
    if (!m || !o || !chains || n_chains < 1) return fail(MOSHII_ERR_ARG, "bad argument");
    bool broken = false;
    int rc = chain_solve_once(m, prior, o, n_chains, chains, flags, (hipStream_t)stream_, &broken);
    if (rc || !broken) return rc;
    // the same solve as plain chains, over whatever the broken groups left in the rows (the first attempt's buffers are gone by now)
    note_coop_broken("moshii_chain_solve");
    return chain_solve_once(m, prior, o, n_chains, chains, (flags & ~0xff00u) | (1u << 8), (hipStream_t)stream_, &broken);
}

int moshii_plan_chunks(int32_t F, int32_t num_chunks, int32_t warmup, int32_t cap, int32_t* starts, int32_t* launch_starts) {
    if (F < 0 || num_chunks < 1 || warmup < 0 || cap < 1 || !starts || !launch_starts) return fail(MOSHII_ERR_ARG, "bad argument");
    return solve_plan::plan_chunks(F, num_chunks, warmup, cap, starts, launch_starts);
}

int moshii_sequence_solve(moshii_model_t m, moshii_prior_t prior, const moshii_solve_opts* o, int32_t n_seq,
                          const moshii_sequence_desc* seqs, const moshii_chunk_opts* co, uint32_t flags, void* stream_,
                          moshii_chunk_report* report) {
    if (!m || !o || !seqs || n_seq < 1) return fail(MOSHII_ERR_ARG, "bad argument");
    SeqSolve s{m, prior, o, n_seq, seqs, co, flags, (hipStream_t)stream_};
    if (s.E > 0 && s.E != m->nshape) return fail(MOSHII_ERR_ARG, "n_shape does not match moshii_model_set_free_shape");
    int rc;
    if ((rc = s.plan()) || (rc = s.prepare()) || (rc = s.stage()) || (rc = s.launch_pass1())) return rc;
    // ---- verify the hand-offs; re-solve the chunks that fail, round by round
    while (true) {
        if ((rc = s.verify())) return rc;
        for (int c = 0; c < s.NC; ++c)
            if (s.chunks[c].pred >= 0 && s.hdev[c] >= MOSHII_HANDOFF_NAN)   // repairing cannot make it verify
                return fail(MOSHII_ERR_NUMERIC, "a chunk hand-off state is NaN");
        if (s.rounds > s.NC + 1)   // every round makes at least the first failing hand-off of a sequence exact: NC rounds is the worst case
            return fail(MOSHII_ERR_NUMERIC, "chunk hand-offs did not verify within the round limit");
        static const int far_frames = []{ const char* e = getenv("MOSHII_FAR_FRAMES"); return e ? atoi(e) : 160; }();
        const solve_plan::Repairs rep = solve_plan::pick_repairs(s.chunks, s.hdev, s.tol, s.rejoin, far_frames);
        if (rep.todo.empty()) break;
        if ((rc = s.repair_round(rep.todo))) return rc;
    }
    return s.finish(report);
}

int moshii_stagei_solve(moshii_model_t m, moshii_prior_t prior, const moshii_stagei_desc* desc, void* stream) {
    if (!m || !desc) return fail(MOSHII_ERR_ARG, "stagei: null model or desc");
    if (!desc->faces || !desc->marker_vids || !desc->m2b || !desc->wt_init || !desc->n_obs || !desc->obs_ids || !desc->obs ||
        !desc->annealing || !desc->pose_ids) return fail(MOSHII_ERR_ARG, "stagei: missing input array");
    S1ModelView mv;
    mv.V = m->V; mv.K = m->K; mv.NB = m->NB; mv.NP = m->NP; mv.body_dof = m->body_dof; mv.hand_dof = m->hand_dof;
    mv.parents = m->d_parents; mv.anc = m->d_anc; mv.vt = m->d_vt; mv.shapedirs = m->d_shapedirs; mv.posedirs = m->d_posedirs;
    mv.weights = m->d_weights; mv.Jreg = m->d_Jreg; mv.hands_mean = m->d_hands_mean; mv.comps = m->d_comps;
    S1PriorView pv;
    if (prior) { pv.G = prior->G; pv.npose = prior->npose; pv.means = prior->d_means; pv.chols = prior->d_chols; pv.neglogw = prior->d_neglogw; }
    char err[256] = {0};
    int rc = moshii_stagei_core(&mv, prior ? &pv : nullptr, desc, stream, err, sizeof(err));
    if (rc != MOSHII_OK) return fail(rc, err);
    return MOSHII_OK;
}

int moshii_last_launch_info(char* kernel_name, int32_t name_cap, int32_t* lds_bytes, int32_t* block_threads) {
    std::lock_guard<std::mutex> hold(g_last_mutex);
    if (kernel_name && name_cap > 0) { strncpy(kernel_name, g_last.name.c_str(), name_cap - 1); kernel_name[name_cap - 1] = 0; }
    if (lds_bytes) *lds_bytes = g_last.lds;
    if (block_threads) *block_threads = g_last.threads;
    return MOSHII_OK;
}

}  // extern "C"

// accessors for lbs_forward.hip (keeps the handle layout private to this file)
extern "C" {
int moshii_internal_model_dims(moshii_model_t m, int* V, int* K) { *V = m->V; *K = m->K; return 0; }
const double* moshii_internal_vsh(moshii_model_t m) { return m->d_vsh; }
const double* moshii_internal_posedirs(moshii_model_t m) { return m->d_posedirs; }
const double* moshii_internal_weights(moshii_model_t m) { return m->d_weights; }
const double* moshii_internal_J(moshii_model_t m) { return m->d_J; }
const double* moshii_internal_weights_host(moshii_model_t m) { return m->weights_host.data(); }
// the free shape block: the device copy of shapedirs [V][3][NB], the block's first column and size, JS [K][nshape][3]
const double* moshii_internal_shape_block(moshii_model_t m, int* NB, int* start, int* count, const double** JS) {
    *NB = m->NB; *start = m->shape_start; *count = m->nshape; *JS = m->d_JS;
    return m->d_shapedirs;
}
void* moshii_internal_l32(moshii_model_t m) { return &m->l32; }
// device buffers for callers without an allocator of their own (moshpp_amd/capi.py: DeviceBuffer)
void* moshii_internal_dev_alloc(size_t bytes) { void* p = nullptr; return hipMalloc((void**)&p, bytes ? bytes : 1) == hipSuccess ? p : nullptr; }
void moshii_internal_dev_free(void* p) { if (p) hipFree(p); }
int moshii_internal_dev_copy(void* dst, const void* src, size_t bytes, int to_device) {
    return hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
void moshii_internal_l32_set_valid(moshii_model_t m, int v) { m->l32_valid = v != 0; }
}

// fql_cfgrl.h -- the kernels of the CFGRL agent (agents/cfgrl.py) that the other headers do not cover: batch assembly with a per-row goal
// vector (given, or drawn from the row's own trajectory as GCDataset.sample_goals does), the per-row Bernoulli mask that replaces the goal
// by the learned unc_embed row, the gradient of that row, the 4-info finalize, and the sampler's input rows and layer 0.  The GEMM bodies,
// weight gradients, LayerNorm backward, the flow-matching loss (fql_loss_bc_body: its 2 / (B act) scaling is this loss's), Adam and the
// grad statistics are FQL's; the sampler's CFG combine, Euler add and final clip are IQL-diffusion's fql_iqld_cfg_step_kernel, unchanged.
// The sweep program (one guidance weight per row) adds fql_cfgrl_cfg_layer0_kernel and ends on IQL-diffusion's rows step kernel.
// Every kernel a CFGRL agent group fuses (fql_cfgrl_group_*) comes in three parts: a __device__ body, the by-value
// entry a single handle launches, and a *_multi_kernel that takes a device array of the same argument struct, one per member.
//
// actor_flow is GCActorVectorField: MLP((*hidden, act), GELU, LayerNorm optional) on [obs | goal | x_t | t], t one column.
#pragma once
#include "fql_iqld.h"

// Info slots while a CFGRL update runs: the loss body writes slot 5 and FQL's finalize slots 10-12; fql_cfgrl_finalize_kernel moves them
// into the reference's order (agents/cfgrl.py:40-56 + utils/flax_utils.py:132-159): actor/actor_loss, grad/max, grad/min, grad/norm
enum : int { CFGRL_I_LOSS = 5, CFGRL_NUM_DRAWS = 6 };
// Philox tensors of the goal draw and the mask (the index draw is tensor 7, x_0 tensor 2 and t tensor 3, as every prep kernel's)
enum : uint32_t { CFGRL_T_RANDOM = 20u, CFGRL_T_DIST = 21u, CFGRL_T_TRAJ = 22u, CFGRL_T_CUR = 23u, CFGRL_T_MASK = 24u };
// rows of the raw-draw read-back [CFGRL_NUM_DRAWS][B]
enum : int { CFGRL_D_IDX = 0, CFGRL_D_RANDOM, CFGRL_D_DIST, CFGRL_D_TRAJ, CFGRL_D_CUR, CFGRL_D_MASK };

// where the goals and the mask of a step come from; rewritten by the host only when it changes (as SrcDesc)
struct CfgrlSrc {
    const float* goals;            // [B, G]: the batch's actor_goals, or null: the goal draw
    const unsigned char* do_cfg;   // [B]: explicit mask, or null: Philox tensor CFGRL_T_MASK
    const int64_t* final_idx;      // [N]: the last row of each row's trajectory (goal draw)
    const float* reps;             // [N, G]: the goal representation of every dataset row (oracle_reps, else the observations)
    int64_t n;                     // dataset rows: the range of the random goal
    double thr_traj;               // p_trajgoal / (1 - p_curgoal)
    double p_cur;
    uint64_t thr_mask;             // do_cfg = u32 < thr_mask, thr_mask = floor(p_uncond 2^32)
    int all_cur;                   // p_curgoal == 1: goal = idx, nothing else is read
};

// utils/datasets.py:224-255 with geom_sample = False, from the four raw 32-bit draws.  Every u32 / 2^32 is exact in a double.  The convex
// combination runs in the reference's order, min(idx + 1, final) d + final (1 - d), each operation rounded on its own: __dmul_rn and
// __dadd_rn are plain operators in this toolchain's headers, which the default -ffp-contract=fast-honor-pragmas may fuse, so the pragma
// below is what keeps a fused multiply-add from deciding which side of .5 the sum lands on.  rint in the default rounding mode is
// np.round's half to even.
__device__ __forceinline__ int64_t cfgrl_goal_index(int64_t idx, int64_t fin, const CfgrlSrc& Gs, uint32_t r_random, uint32_t r_dist,
                                                    uint32_t r_traj, uint32_t r_cur) {
#pragma clang fp contract(off)
    if (Gs.all_cur) return idx;
    const double inv = 1.0 / 4294967296.0;
    const int64_t random_goal = (int64_t)(((uint64_t)r_random * (uint64_t)Gs.n) >> 32);
    const double d = (double)r_dist * inv;
    const int64_t m = idx + 1 < fin ? idx + 1 : fin;
    const double lhs = (double)m * d;
    const double om = 1.0 - d;
    const double rhs = (double)fin * om;
    const double s = lhs + rhs;
    const int64_t traj_goal = (int64_t)rint(s);
    int64_t g = ((double)r_traj * inv < Gs.thr_traj) ? traj_goal : random_goal;
    if ((double)r_cur * inv < Gs.p_cur) g = idx;
    return g;
}

struct CfgrlPrepArgs {
    const SrcDesc* src;
    const CfgrlSrc* gsrc;
    DevState* st;
    uint64_t key;
    const float* unc;          // [G]: modules_unc_embed/Embed_0/embedding of the current parameters
    int B, od, G, ad;
    int inp, ap;               // padded input width of actor_flow (od + G + ad + 1), padded action width
    float *X, *vel;            // [B, inp], [B, ap]
    int64_t* rows;             // [2][B]: idx, goal_idx (-1 when the goals came with the batch)
    uint32_t* draws;           // [CFGRL_NUM_DRAWS][B]: the raw draws (0 where a draw was not made)
    unsigned char* mask;       // [B]: do_cfg
};
// utils/datasets.py:64-100 (index draw + gather) and :224-255 (goal), agents/cfgrl.py:24-37 (x_0, t, x_t, vel, do_cfg, goals): one wave
// per transition writes X = [obs | goal or unc_embed | x_t | t | 0] and vel = act - x_0.  x_0 is Philox tensor 2 and t tensor 3 (continuous,
// as IFQL's); explicit tensors replace them.
__device__ __forceinline__ void fql_cfgrl_prep_body(const CfgrlPrepArgs& P) {
    const SrcDesc& S = *P.src;
    const CfgrlSrc& Gs = *P.gsrc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= P.B) return;
    const uint64_t step = P.st->rng_step;
    const uint64_t key = P.key ^ (P.st->rng_stream * 0x9E3779B97F4A7C15ull);
    uint32_t r[CFGRL_NUM_DRAWS] = {0u, 0u, 0u, 0u, 0u, 0u};
    int64_t src = b;
    if (S.idx) src = S.idx[b];
    else if (S.use_rng_idx) {
        r[CFGRL_D_IDX] = rng_u32(key, step, 7u, (uint32_t)b);
        src = S.lo + (int64_t)(((uint64_t)r[CFGRL_D_IDX] * (uint64_t)S.span) >> 32);
    }
    const int od = P.od, G = P.G, ad = P.ad;
    int64_t gi = -1;
    const float* goal;
    if (Gs.goals) goal = Gs.goals + (size_t)b * G;
    else {
        if (!Gs.all_cur) {
            r[CFGRL_D_RANDOM] = rng_u32(key, step, CFGRL_T_RANDOM, (uint32_t)b);
            r[CFGRL_D_DIST] = rng_u32(key, step, CFGRL_T_DIST, (uint32_t)b);
            r[CFGRL_D_TRAJ] = rng_u32(key, step, CFGRL_T_TRAJ, (uint32_t)b);
            r[CFGRL_D_CUR] = rng_u32(key, step, CFGRL_T_CUR, (uint32_t)b);
        }
        gi = cfgrl_goal_index(src, Gs.final_idx[src], Gs, r[CFGRL_D_RANDOM], r[CFGRL_D_DIST], r[CFGRL_D_TRAJ], r[CFGRL_D_CUR]);
        goal = Gs.reps + (size_t)gi * G;
    }
    bool drop;
    if (Gs.do_cfg) drop = Gs.do_cfg[b] != 0;
    else {
        r[CFGRL_D_MASK] = rng_u32(key, step, CFGRL_T_MASK, (uint32_t)b);
        drop = (uint64_t)r[CFGRL_D_MASK] < Gs.thr_mask;
    }
    if (drop) goal = P.unc;                                      // cfgrl.py:35
    const float* obs = S.obs + (size_t)src * od;
    const float* act = S.act + (size_t)src * ad;
    const float tt = S.t ? S.t[b] : rng_uniform(key, step, 3u, (uint32_t)b);
    const int a0 = od + G, t0 = a0 + ad;
    for (int j = lane; j < P.inp; j += 64) {
        float v = 0.f;
        if (j < od) v = obs[j];
        else if (j < a0) v = goal[j - od];
        else if (j < t0) {
            const int a = j - a0;
            const float av = act[a];
            const float xx = S.x0 ? S.x0[(size_t)b * ad + a] : rng_normal(key, step, 2u, (uint32_t)b, (uint32_t)a);
            v = (1.0f - tt) * xx + tt * av;                      // cfgrl.py:30
            P.vel[(size_t)b * P.ap + a] = av - xx;               // cfgrl.py:31
        } else if (j == t0) v = tt;
        P.X[(size_t)b * P.inp + j] = v;
    }
    if (lane == 0) {
        P.rows[b] = src;
        P.rows[(size_t)P.B + b] = gi;
        P.mask[b] = drop ? 1 : 0;
    }
    if (lane < CFGRL_NUM_DRAWS) {
        uint32_t v = r[0];
#pragma unroll
        for (int i = 1; i < CFGRL_NUM_DRAWS; ++i) v = lane == i ? r[i] : v;
        P.draws[(size_t)lane * P.B + b] = v;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_prep_kernel(CfgrlPrepArgs P) { fql_cfgrl_prep_body(P); }
// Multi-instance entry points (CFGRL agent groups), here and below: blockIdx.y picks the member, its argument struct comes from a device
// array, read through the constant address space (scalar loads, as from the kernel-argument segment; fql_kernels.h FQL_CONST_AS).
// Shared-memory arrays are declared in the entries and handed to the body: the single-workgroup kernels run as grid (1, members), each
// workgroup the member's own fixed-order reduction.
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_prep_multi_kernel(const CfgrlPrepArgs* __restrict__ args) { const CfgrlPrepArgs P = ((const FQL_CONST_AS CfgrlPrepArgs*)args)[blockIdx.y]; fql_cfgrl_prep_body(P); }

struct CfgrlEmbedGradArgs {
    const float* dZ0;          // [B, H]: gradient at layer 0's pre-activation
    const float* W0g;          // row od of W0 [in_p, H]: the G goal rows
    const unsigned char* mask; // [B]: do_cfg
    float* g;                  // [G]: the gradient slot of modules_unc_embed/Embed_0/embedding
    int B, H, G;
};
// The goal columns of every dropped row hold the one unc_embed row, so dU = (column sum of dZ0 over the dropped rows) W0[goal rows]^T
// (cfgrl.py:33-37: the where sends no gradient through the kept rows).  One workgroup.  Per chunk of 256 rows the dropped rows' indices are
// compacted into LDS in rising order (ballot + prefix count), so the column sums read only those rows - a tenth of the batch - with no
// load of the mask inside the sum: a loop over every row that tests mask[b] first costs one dependent global load per row (measured: 80 us
// at B 256).  Each thread owns columns threadIdx.x + 256 i, i < 4 (H <= 1024), and adds the rows in rising b, eight loads in flight.  Then one wave per goal
// column, the products over h in rising order per lane and a fixed shuffle tree over the lanes.  No dropped row: every sum stays 0.f, dU
// is exactly zero.  cs: [1024], rows: [FQL_THREADS], cnt: [FQL_THREADS / 64] in LDS.
__device__ __forceinline__ void fql_cfgrl_embed_grad_body(const CfgrlEmbedGradArgs& P, float* cs, int* rows, int* cnt) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < P.B; b0 += FQL_THREADS) {
        const int b = b0 + (int)threadIdx.x;
        const bool drop = b < P.B && P.mask[b] != 0;
        const unsigned long long bal = __ballot(drop);
        if (lane == 0) cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FQL_THREADS / 64; ++w) {
            off += w < wave ? cnt[w] : 0;
            total += cnt[w];
        }
        if (drop) rows[off + __popcll(bal & ((1ull << lane) - 1ull))] = b;
        __syncthreads();
        for (int k = 0; k < total; k += 8) {   // eight rows' loads in flight, then added in rising b (a row past the list adds 0.f)
            float v[8][4];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool live = k + u < total;
                const float* r = P.dZ0 + (size_t)rows[live ? k + u : k] * P.H;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int h = (int)threadIdx.x + FQL_THREADS * i;
                    v[u][i] = live && h < P.H ? r[h] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] += v[u][i];
        }
        __syncthreads();   // rows and cnt are rewritten by the next chunk
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int h = (int)threadIdx.x + FQL_THREADS * i;
        if (h < P.H) cs[h] = s[i];
    }
    __syncthreads();
    for (int j = wave; j < P.G; j += FQL_THREADS / 64) {
        const float* w = P.W0g + (size_t)j * P.H;
        float t = 0.f;
        for (int h = lane; h < P.H; h += 64) t = fmaf(cs[h], w[h], t);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o);
        if (lane == 0) P.g[j] = t;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_embed_grad_kernel(CfgrlEmbedGradArgs P) { __shared__ float cs[1024]; __shared__ int rows[FQL_THREADS]; __shared__ int cnt[FQL_THREADS / 64]; fql_cfgrl_embed_grad_body(P, cs, rows, cnt); }
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_embed_grad_multi_kernel(const CfgrlEmbedGradArgs* __restrict__ args) { __shared__ float cs[1024]; __shared__ int rows[FQL_THREADS]; __shared__ int cnt[FQL_THREADS / 64]; const CfgrlEmbedGradArgs P = ((const FQL_CONST_AS CfgrlEmbedGradArgs*)args)[blockIdx.y]; fql_cfgrl_embed_grad_body(P, cs, rows, cnt); }

// FQL's finalize (grad statistics into slots 10-12 and the step counters), then the reference's order in slots 0-3
__device__ __forceinline__ void fql_cfgrl_finalize_body(const FinalizeArgs& A) {
    fql_finalize_body(A);
    if (threadIdx.x == 0) {
        float* in = A.st->info;
        const float loss = in[CFGRL_I_LOSS], gmax = in[10], gmin = in[11], gn = in[12];
        in[0] = loss; in[1] = gmax; in[2] = gmin; in[3] = gn;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_finalize_kernel(FinalizeArgs A) { fql_cfgrl_finalize_body(A); }
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_finalize_multi_kernel(const FinalizeArgs* __restrict__ args) { const FinalizeArgs A = ((const FQL_CONST_AS FinalizeArgs*)args)[blockIdx.y]; fql_cfgrl_finalize_body(A); }

// ---- sample_actions (agents/cfgrl.py:70-100) ---------------------------------------------------------------------------------------
// IQL-diffusion's two-half form: rows [0, n_pad) are the conditional pass ([obs | goal]), rows [n_pad, 2 n_pad) the unconditional one
// ([obs | unc_embed]); both read the same x.  Layer 0 of step i is z0 = C0 + x W0[act rows] + (i / S) W0[t row] with the loop-invariant
// C0 = [obs | goal] W0[obs and goal rows] + b0 (one GEMM over both halves per call): t is one column, so a step needs no bias table.
struct CfgrlAssembleArgs {
    const float *obs, *goals, *unc, *noise;   // obs [n, od]; goals [n, G]; unc [G]: the unc_embed row; noise [n, ad] or null
    float* X;                  // [2 n_pad, inp]: row r = [obs_r | goal_r | 0], row n_pad + r = [obs_r | unc | 0]; rows >= n of a half are zero
    float* A;                  // [n_pad, ap]: x_r (the flow's state); padding columns and rows >= n are zero
    uint64_t key, seed;
    int n, n_pad, od, G, ad, inp, ap;
    int row0;                  // index of this chunk's first row in the call (keys the Philox draw: chunking does not change the noise)
};
__device__ __forceinline__ void fql_cfgrl_assemble_body(const CfgrlAssembleArgs& P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= P.n_pad) return;
    const bool live = r < P.n;
    const float* goal = P.goals + (size_t)r * P.G;
    for (int j = lane; j < P.inp; j += 64) {
        float c = 0.f, u = 0.f;
        if (live && j < P.od) c = u = P.obs[(size_t)r * P.od + j];
        else if (live && j < P.od + P.G) { c = goal[j - P.od]; u = P.unc[j - P.od]; }
        P.X[(size_t)r * P.inp + j] = c;
        P.X[(size_t)(P.n_pad + r) * P.inp + j] = u;
    }
    for (int a = lane; a < P.ap; a += 64) {
        float v = 0.f;
        if (live && a < P.ad) v = P.noise ? P.noise[(size_t)r * P.ad + a] : rng_normal(P.key, P.seed, 12u, (uint32_t)(P.row0 + r), (uint32_t)a);
        P.A[(size_t)r * P.ap + a] = v;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_assemble_kernel(CfgrlAssembleArgs P) { fql_cfgrl_assemble_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_assemble_multi_kernel(const CfgrlAssembleArgs* __restrict__ args) { const CfgrlAssembleArgs P = ((const FQL_CONST_AS CfgrlAssembleArgs*)args)[blockIdx.y]; fql_cfgrl_assemble_body(P); }

struct CfgrlLayer0Args {
    const float *C0, *A, *W0a;   // C0 [2 n_pad, H]; A [n_pad, ap]; W0a = row od + G of W0 [in_p, H]: ad action rows, then the t row
    float* G0;                   // [2 n_pad, H]
    int n_pad, H, ad, ap;
    float t;                     // i / flow_steps
};
// layer 0 of one Euler step for both halves: one thread per (row, column), the act terms in fixed order, then the t term
__device__ __forceinline__ void fql_cfgrl_layer0_body(const CfgrlLayer0Args& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= 2 * P.n_pad * P.H) return;
    const int r = e / P.H, h = e - r * P.H;
    const int src = r >= P.n_pad ? r - P.n_pad : r;
    float s = P.C0[e];
    const float* x = P.A + (size_t)src * P.ap;
    for (int a = 0; a < P.ad; ++a) s = fmaf(x[a], P.W0a[(size_t)a * P.H + h], s);
    s = fmaf(P.t, P.W0a[(size_t)P.ad * P.H + h], s);
    P.G0[e] = gelu_f(s);
}
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_layer0_kernel(CfgrlLayer0Args P) { fql_cfgrl_layer0_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_layer0_multi_kernel(const CfgrlLayer0Args* __restrict__ args) { const CfgrlLayer0Args P = ((const FQL_CONST_AS CfgrlLayer0Args*)args)[blockIdx.y]; fql_cfgrl_layer0_body(P); }

struct CfgrlCfgLayer0Args {
    const float *C0, *V, *Xin, *cfg, *W0a;   // C0 [2 n_pad, H]; V [2 n_pad, ap]: the previous step's head output; Xin [n_pad, ap]; cfg [n_pad];
                                             // W0a = row od + G of W0 [in_p, H]: ad action rows, then the t row
    float *Xout, *G0;                        // Xout [n_pad, ap]: the other ping-pong buffer; G0 [2 n_pad, H]
    int n_pad, H, ad, ap;
    float t, dt;                             // i / flow_steps; 1 / flow_steps
};
// Euler step i >= 1 of a sweep program (sample_actions_cfgs) in one launch: fql_iqld_cfg_layer0_kernel around fql_cfgrl_layer0_kernel's
// layer 0 (C0 spans both halves; the act terms in rising order, then the t term)
// (the body takes the struct by value: through a reference the by-value entry compiles to 28 SGPRs, this way to the 26 it had as one
// function)
__device__ __forceinline__ void fql_cfgrl_cfg_layer0_body(const CfgrlCfgLayer0Args P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= 2 * P.n_pad * P.H) return;
    const int r = e / P.H, h = e - r * P.H;
    const int half = r >= P.n_pad ? 1 : 0, src = r - half * P.n_pad;
    float s = P.C0[e];
    const float* x = P.Xin + (size_t)src * P.ap;
    const float* vp = P.V + (size_t)src * P.ap;
    const float* vu = P.V + (size_t)(P.n_pad + src) * P.ap;
    const float c = P.cfg[src];
    for (int a = 0; a < P.ad; ++a) s = fmaf(iqld_cfg_euler(x[a], vp[a], vu[a], c, P.dt), P.W0a[(size_t)a * P.H + h], s);
    s = fmaf(P.t, P.W0a[(size_t)P.ad * P.H + h], s);
    P.G0[e] = gelu_f(s);
    if (half == 0)
        for (int a = h; a < P.ap; a += P.H)
            P.Xout[(size_t)src * P.ap + a] = a < P.ad ? iqld_cfg_euler(x[a], vp[a], vu[a], c, P.dt) : 0.f;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_cfg_layer0_kernel(CfgrlCfgLayer0Args P) { fql_cfgrl_cfg_layer0_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_cfgrl_cfg_layer0_multi_kernel(const CfgrlCfgLayer0Args* __restrict__ args) { const CfgrlCfgLayer0Args P = ((const FQL_CONST_AS CfgrlCfgLayer0Args*)args)[blockIdx.y]; fql_cfgrl_cfg_layer0_body(P); }

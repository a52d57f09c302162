// fql_ifql.h -- the kernels of the IFQL agent (agents/ifql.py) that FQL's kernels do not cover: batch assembly, the IQL value and
// critic losses, the info layout of the finalize step, and best-of-N action selection.  The GEMM bodies, weight gradients,
// LayerNorm backward, the flow-matching loss (fql_loss_bc_body), Adam + Polyak and the grad statistics are FQL's.
// Every kernel an IFQL agent group fuses (fql_ifql_group_*) comes in three parts: a __device__ body, the by-value
// entry a single handle launches, and a *_multi_kernel that takes a device array of the same argument struct, one per member.
#pragma once
#include "fql_kernels.h"

// Info slots while an IFQL update runs (the BC loss body writes slot 5, as in FQL); fql_ifql_finalize_kernel moves them into the
// reference's order (agents/ifql.py:79-98 + utils/flax_utils.py:151-157):
//   value_loss, v_mean, v_max, v_min, critic_loss, q_mean, q_max, q_min, actor_loss, grad/max, grad/min, grad/norm, 0
enum : int { IFQL_I_VALUE = 0, IFQL_I_CRITIC = 4, IFQL_I_ACTOR = 5, IFQL_I_Q = 6 };

struct IfqlPrepArgs {
    const SrcDesc* src;
    DevState* st;
    uint64_t key;
    int B, od, ad;
    int inp_v, inp_c, inp_b, ap;   // padded input widths: value (od), critic (od + ad), actor_flow (od + ad + 1); action width
    float *X_v, *X_c, *X_bc, *vel, *w_rew, *w_mask;
};
// utils/datasets.py:64-100 (index draw + gather), agents/ifql.py:62-69 (x_0, t, x_t, vel): one wave per transition builds
// X_v = [obs ; next_obs] (2B rows), X_c = [obs | act], X_bc = [obs | x_t | t], vel = act - x_0.  x_0 and t are the same Philox tensors
// (2, 3) as FQL's BC-flow noise; explicit tensors replace them.
__device__ __forceinline__ void fql_ifql_prep_body(const IfqlPrepArgs& P) {
    const SrcDesc& S = *P.src;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= P.B) return;
    const uint64_t step = P.st->rng_step;
    const uint64_t key = P.key ^ (P.st->rng_stream * 0x9E3779B97F4A7C15ull);
    int64_t src = b;
    if (S.idx) src = S.idx[b];
    else if (S.use_rng_idx) src = S.lo + (int64_t)(((uint64_t)rng_u32(key, step, 7u, (uint32_t)b) * (uint64_t)S.span) >> 32);
    const int od = P.od, ad = P.ad, B = P.B;
    const float* obs = S.obs + (size_t)src * od;
    const float* nobs = S.nobs + (size_t)src * od;
    const float* act = S.act + (size_t)src * ad;
    const float tt = S.t ? S.t[b] : rng_uniform(key, step, 3u, (uint32_t)b);
    int w = P.inp_v > P.inp_c ? P.inp_v : P.inp_c;
    w = w > P.inp_b ? w : P.inp_b;
    for (int j = lane; j < w; j += 64) {
        const bool is_obs = j < od, is_act = j >= od && j < od + ad;
        const int a = j - od;
        const float o = is_obs ? obs[j] : 0.f;
        float av = 0.f, xx = 0.f;
        if (is_act) {
            av = act[a];
            xx = S.x0 ? S.x0[(size_t)b * ad + a] : rng_normal(key, step, 2u, (uint32_t)b, (uint32_t)a);
        }
        if (j < P.inp_v) {
            P.X_v[(size_t)b * P.inp_v + j] = o;                                   // value(obs)       ifql.py:34
            P.X_v[(size_t)(B + b) * P.inp_v + j] = is_obs ? nobs[j] : 0.f;        // value(next_obs)  ifql.py:47
        }
        if (j < P.inp_c) P.X_c[(size_t)b * P.inp_c + j] = is_act ? av : o;        // (target_)critic(obs, actions)  ifql.py:33,50
        if (j < P.inp_b) P.X_bc[(size_t)b * P.inp_b + j] = is_obs ? o : (is_act ? (1.0f - tt) * xx + tt * av : (j == od + ad ? tt : 0.f));  // ifql.py:68
        if (is_act) P.vel[(size_t)b * P.ap + a] = av - xx;                       // ifql.py:69
    }
    if (lane == 0) {
        P.w_rew[b] = S.rew[src];
        P.w_mask[b] = S.mask[src];
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_prep_kernel(IfqlPrepArgs P) { fql_ifql_prep_body(P); }
// Multi-instance entry points (IFQL agent groups; the value loss below also IQL-diffusion's), here and below: blockIdx.y picks the member,
// its argument struct comes from a device array, read through the constant address space (scalar loads, as from the kernel-argument
// segment; fql_kernels.h FQL_CONST_AS).  Shared-memory arrays are declared in the entries and handed to the body.  Grid x = rows / 4.
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_prep_multi_kernel(const IfqlPrepArgs* __restrict__ args) { const IfqlPrepArgs P = ((const FQL_CONST_AS IfqlPrepArgs*)args)[blockIdx.y]; fql_ifql_prep_body(P); }

struct IfqlValueArgs {
    const float* v;            // [B, 16] column 0: value(obs) (rows 0..B-1 of the [obs ; next_obs] pass)
    const float *tqa, *tqb;    // [B, 16] column 0: target critic members at (obs, act)
    float* dv;                 // [B, 16] column 0 or null
    DevState* st;
    int B;
    float expectile;
};
// agents/ifql.py:25-43: q = min(target q1, q2); loss = mean(w (q - v)^2), w = expectile where q - v >= 0, else 1 - expectile
__device__ __forceinline__ void fql_ifql_loss_value_body(const IfqlValueArgs& P, float* sh) {
    const float gs = 2.0f / (float)P.B;
    float sl = 0.f, sv = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float v = P.v[(size_t)b * 16];
        const float q = fminf(P.tqa[(size_t)b * 16], P.tqb[(size_t)b * 16]);
        const float d = q - v;
        const float w = d >= 0.f ? P.expectile : 1.0f - P.expectile;
        sl += w * d * d;
        sv += v;
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
        if (P.dv) P.dv[(size_t)b * 16] = -gs * w * d;
    }
    const float tl = block_sum(sl, sh), tv = block_sum(sv, sh);
    const float tmx = block_max(mx, sh), tmn = -block_max(-mn, sh);
    if (threadIdx.x == 0) {
        float* in = P.st->info + IFQL_I_VALUE;
        in[0] = tl / (float)P.B;
        in[1] = tv / (float)P.B;
        in[2] = tmx;
        in[3] = tmn;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_loss_value_kernel(IfqlValueArgs P) { __shared__ float sh[4]; fql_ifql_loss_value_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_loss_value_multi_kernel(const IfqlValueArgs* __restrict__ args) { __shared__ float sh[4]; const IfqlValueArgs P = ((const FQL_CONST_AS IfqlValueArgs*)args)[blockIdx.y]; fql_ifql_loss_value_body(P, sh); }

struct IfqlCriticArgs {
    const float* nv;           // [B, 16] column 0: value(next_obs) with the stored parameters (rows B..2B-1 of the value pass)
    const float *qa, *qb;      // [B, 16] column 0: critic members at (obs, act)
    const float *w_rew, *w_mask;
    float *dqa, *dqb;          // [B, 16] column 0 or null
    DevState* st;
    int B;
    float discount;
};
// agents/ifql.py:45-58: y = r + discount mask v(next_obs); loss = mean((q1 - y)^2 + (q2 - y)^2) (a SUM over the two members);
// q_mean / q_max / q_min are statistics of y
__device__ __forceinline__ void fql_ifql_loss_critic_body(const IfqlCriticArgs& P, float* sh) {
    const float gs = 2.0f / (float)P.B;
    float sl = 0.f, sy = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float y = P.w_rew[b] + P.discount * P.w_mask[b] * P.nv[(size_t)b * 16];
        const float da = P.qa[(size_t)b * 16] - y, db = P.qb[(size_t)b * 16] - y;
        sl += da * da + db * db;
        sy += y;
        mx = fmaxf(mx, y);
        mn = fminf(mn, y);
        if (P.dqa) {
            P.dqa[(size_t)b * 16] = gs * da;
            P.dqb[(size_t)b * 16] = gs * db;
        }
    }
    const float tl = block_sum(sl, sh), ty = block_sum(sy, sh);
    const float tmx = block_max(mx, sh), tmn = -block_max(-mn, sh);
    if (threadIdx.x == 0) {
        P.st->info[IFQL_I_CRITIC] = tl / (float)P.B;
        P.st->info[IFQL_I_Q] = ty / (float)P.B;
        P.st->info[IFQL_I_Q + 1] = tmx;
        P.st->info[IFQL_I_Q + 2] = tmn;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_loss_critic_kernel(IfqlCriticArgs P) { __shared__ float sh[4]; fql_ifql_loss_critic_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_loss_critic_multi_kernel(const IfqlCriticArgs* __restrict__ args) { __shared__ float sh[4]; const IfqlCriticArgs P = ((const FQL_CONST_AS IfqlCriticArgs*)args)[blockIdx.y]; fql_ifql_loss_critic_body(P, sh); }

// FQL's finalize (grad statistics into slots 10-12 and the step counters when A.do_grad_stats), then the reference's IFQL order
// (fql_finalize_body declares the LDS it needs itself, sh[4] and leafn[256]: both entries get it through the inlined body)
__device__ __forceinline__ void fql_ifql_finalize_body(const FinalizeArgs& A) {
    fql_finalize_body(A);
    if (threadIdx.x == 0) {
        float* in = A.st->info;
        const float actor = in[IFQL_I_ACTOR], qm = in[IFQL_I_Q], qx = in[IFQL_I_Q + 1], qn = in[IFQL_I_Q + 2];
        const float gmax = A.do_grad_stats ? in[10] : 0.f, gmin = A.do_grad_stats ? in[11] : 0.f, gn = A.do_grad_stats ? in[12] : 0.f;
        in[5] = qm; in[6] = qx; in[7] = qn; in[8] = actor;
        in[9] = gmax; in[10] = gmin; in[11] = gn; in[12] = 0.f;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_finalize_kernel(FinalizeArgs A) { fql_ifql_finalize_body(A); }
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_finalize_multi_kernel(const FinalizeArgs* __restrict__ args) { const FinalizeArgs A = ((const FQL_CONST_AS FinalizeArgs*)args)[blockIdx.y]; fql_ifql_finalize_body(A); }

// ---- sample_actions (agents/ifql.py:123-155) ------------------------------------------------------------------------------------
struct IfqlRepeatArgs {
    const float *obs, *noise;  // obs [n, od]; noise [n * N, ad] or null (Philox keyed by (key, seed))
    float* X;                  // [n_pad, inp]: row i N + k = [obs_i | noise_ik | 0]
    uint64_t key, seed;
    int n, N, n_pad, od, ad, inp;
    int row0;                  // index of this chunk's first row in the call (keys the Philox draw: chunking does not change the noise)
};
__device__ __forceinline__ void fql_ifql_repeat_body(const IfqlRepeatArgs& P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= P.n_pad) return;
    const int i = r / P.N;
    for (int j = lane; j < P.inp; j += 64) {
        float v = 0.f;
        if (r < P.n * P.N) {
            if (j < P.od) v = P.obs[(size_t)i * P.od + j];
            else if (j < P.od + P.ad) {
                const int a = j - P.od;
                v = P.noise ? P.noise[(size_t)r * P.ad + a] : rng_normal(P.key, P.seed, 10u, (uint32_t)(P.row0 + r), (uint32_t)a);
            }
        }
        P.X[(size_t)r * P.inp + j] = v;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_repeat_kernel(IfqlRepeatArgs P) { fql_ifql_repeat_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_repeat_multi_kernel(const IfqlRepeatArgs* __restrict__ args) { const IfqlRepeatArgs P = ((const FQL_CONST_AS IfqlRepeatArgs*)args)[blockIdx.y]; fql_ifql_repeat_body(P); }
// critic input [obs_i | clip(flow action)] of every sample row
struct IfqlQinArgs {
    const float *obs, *act;    // obs [n, od]; act [n_pad, ap] (clipped Euler result)
    float* X;                  // [n_pad, inp]
    int n, N, n_pad, od, ad, ap, inp;
};
__device__ __forceinline__ void fql_ifql_qin_body(const IfqlQinArgs& P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= P.n_pad) return;
    const int i = r / P.N;
    for (int j = lane; j < P.inp; j += 64) {
        float v = 0.f;
        if (r < P.n * P.N) {
            if (j < P.od) v = P.obs[(size_t)i * P.od + j];
            else if (j < P.od + P.ad) v = P.act[(size_t)r * P.ap + (j - P.od)];
        }
        P.X[(size_t)r * P.inp + j] = v;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_qin_kernel(IfqlQinArgs P) { fql_ifql_qin_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_qin_multi_kernel(const IfqlQinArgs* __restrict__ args) { const IfqlQinArgs P = ((const FQL_CONST_AS IfqlQinArgs*)args)[blockIdx.y]; fql_ifql_qin_body(P); }
// best of N: q = min over the two critic members, the FIRST index of the largest q (jnp.argmax), its action.  One wave per observation
// (wave64: the butterfly covers offsets 32 .. 1, cdna_hip_programming.md section 1); ties resolve to the lower index at every step.
struct IfqlSelectArgs {
    const float *qa, *qb;      // [n_pad, 16] column 0
    const float* act;          // [n_pad, ap]
    float* out;                // [n, ad]
    int n, N, ad, ap;
};
__device__ __forceinline__ void fql_ifql_select_body(const IfqlSelectArgs& P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= P.n) return;
    float best = -INFINITY;
    int bi = 0x7FFFFFFF;
    for (int k = lane; k < P.N; k += 64) {
        const size_t r = (size_t)i * P.N + k;
        const float q = fminf(P.qa[r * 16], P.qb[r * 16]);
        if (q > best || bi == 0x7FFFFFFF) { best = q; bi = k; }   // (k rises within a lane: the first maximum is kept)
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi == 0x7FFFFFFF) bi = 0;
    for (int a = lane; a < P.ad; a += 64) P.out[(size_t)i * P.ad + a] = P.act[((size_t)i * P.N + bi) * P.ap + a];
}
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_select_kernel(IfqlSelectArgs P) { fql_ifql_select_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_ifql_select_multi_kernel(const IfqlSelectArgs* __restrict__ args) { const IfqlSelectArgs P = ((const FQL_CONST_AS IfqlSelectArgs*)args)[blockIdx.y]; fql_ifql_select_body(P); }

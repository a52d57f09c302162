// fql_iql.h -- the kernels of the IQL agent (agents/iql.py) that the other headers do not cover: batch assembly, the plain (unsquashed)
// Gaussian actor's log-probability, its two losses (AWR and DDPG+BC) with the gradients handed to the actor's mean head and to the
// log_stds vector, the info layout of the finalize step and the sampling head.  The value and critic losses are IFQL's
// (fql_ifql_loss_value_kernel, fql_ifql_loss_critic_kernel: agents/iql.py:28-55 is agents/ifql.py:31-58 term for term); the GEMM bodies,
// weight gradients, LayerNorm backward, the critic's input gradient, Adam + Polyak and the grad statistics are FQL's.  Every reduction
// runs in one workgroup in a fixed order (no float atomics).
// Every kernel an IQL agent group fuses (fql_iql_group_*) comes in three parts: a __device__ body, the by-value
// entry a single handle launches, and a *_multi_kernel that takes a device array of the same argument struct, one per member.
//
// The actor (utils/networks.py:82-150 with state_dependent_std=False) is actor_net + mean_net as one MLP obs -> [B, ap]; log_stds is a
// vector leaf [act] of the arena (const_std=False) or absent (const_std=True: log-std 0).  No tanh squash.
#pragma once
#include "fql_ifql.h"

// Infos of an IQL handle live in a buffer of their own (DevState::info holds 16 floats; ddpgbc has 19 infos).  The value / critic loss
// kernels write DevState::info in IFQL's scratch order; the actor loss kernels write their infos at IQL_I_ACTOR of the IQL buffer and
// fql_iql_finalize_kernel completes it in the reference's order (agents/iql.py:35-40,50-55,74-80,101-110 + utils/flax_utils.py:151-157):
//   value_loss, v_mean, v_max, v_min, critic_loss, q_mean, q_max, q_min,
//   awr:    actor_loss, adv, bc_log_prob, mse, std,                                   grad/max, grad/min, grad/norm   (16)
//   ddpgbc: actor_loss, q_loss, bc_loss, q_mean, q_abs_mean, bc_log_prob, mse, std,    grad/max, grad/min, grad/norm   (19)
enum : int { IQL_I_ACTOR = 8, IQL_N_AWR = 5, IQL_N_DDPGBC = 8, IQL_INFO_STRIDE = 32 };
#define IQL_LOG_STD_MIN (-5.0f)
#define IQL_LOG_STD_MAX 2.0f

__device__ __forceinline__ float iql_clip_ls(float raw) { return fminf(fmaxf(raw, IQL_LOG_STD_MIN), IQL_LOG_STD_MAX); }
// d clip(raw, -5, 2) / d raw as jnp.clip's max / min give it: 1 inside, 0 outside, 1/2 at a bound
__device__ __forceinline__ float iql_ls_mask(float raw) {
    return (raw > IQL_LOG_STD_MIN && raw < IQL_LOG_STD_MAX) ? 1.0f : ((raw == IQL_LOG_STD_MIN || raw == IQL_LOG_STD_MAX) ? 0.5f : 0.0f);
}

struct IqlPrepArgs {
    const SrcDesc* src;
    DevState* st;
    uint64_t key;
    int B, od, ad;
    int inp_v, inp_c, inp_a, ap;   // padded input widths: value (od), critic (od + ad), actor (od); action width
    float *X_v, *X_c, *X_a;        // [2B, inp_v] = [obs ; next_obs], [B, inp_c] = [obs | act], [B, inp_a] = obs
    float* X_q;                    // ddpgbc: [B, inp_c] = [obs | .] (action block: fql_iql_head_kernel), else null
    float *w_act, *w_eps;          // [B, ap]: actions; raw N(0, 1) of dist.sample (ddpgbc with log_stds), else null
    float *w_rew, *w_mask;
};
// utils/datasets.py:64-100 (index draw + gather) and the network inputs of agents/iql.py; eps is fql_noise.eps1 or Philox tensor 1.
// One wave per transition.
// (the body takes the struct by value: through a reference the by-value entry compiles to 66 VGPRs and 7 waves per SIMD, this way to the
// 63 and 8 it had as one function)
__device__ __forceinline__ void fql_iql_prep_body(const IqlPrepArgs P) {
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
    int w = P.inp_v > P.inp_c ? P.inp_v : P.inp_c;
    w = w > P.inp_a ? w : P.inp_a;
    for (int j = lane; j < w; j += 64) {
        const bool is_obs = j < od, is_act = j >= od && j < od + ad;
        const int a = j - od;
        const float o = is_obs ? obs[j] : 0.f;
        const float av = is_act ? act[a] : 0.f;
        if (j < P.inp_v) {
            P.X_v[(size_t)b * P.inp_v + j] = o;                               // value(obs)       iql.py:32,61
            P.X_v[(size_t)(B + b) * P.inp_v + j] = is_obs ? nobs[j] : 0.f;    // value(next_obs)  iql.py:44
        }
        if (j < P.inp_c) {
            P.X_c[(size_t)b * P.inp_c + j] = is_act ? av : o;                 // (target_)critic(obs, actions)  iql.py:30,47,62
            if (P.X_q) P.X_q[(size_t)b * P.inp_c + j] = o;                    // critic(obs, q_actions)  iql.py:90
        }
        if (j < P.inp_a) P.X_a[(size_t)b * P.inp_a + j] = o;                  // actor(obs)  iql.py:69,85
        if (is_act) {
            P.w_act[(size_t)b * P.ap + a] = av;
            if (P.w_eps) P.w_eps[(size_t)b * P.ap + a] = S.eps1 ? S.eps1[(size_t)b * ad + a] : rng_normal(key, step, 1u, (uint32_t)b, (uint32_t)a);
        }
    }
    if (lane == 0) {
        P.w_rew[b] = S.rew[src];
        P.w_mask[b] = S.mask[src];
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_prep_kernel(IqlPrepArgs P) { fql_iql_prep_body(P); }
// Multi-instance entry points (IQL agent groups), here and below: blockIdx.y picks the member, its argument struct comes from a device
// array, read through the constant address space (scalar loads, as from the kernel-argument segment; fql_kernels.h FQL_CONST_AS).
// Shared-memory arrays are declared in the entries and handed to the body: the single-workgroup kernels run as grid (1, members), each
// workgroup the member's own fixed-order reduction.  Grid x = rows / 4.
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_prep_multi_kernel(const IqlPrepArgs* __restrict__ args) { const IqlPrepArgs P = ((const FQL_CONST_AS IqlPrepArgs*)args)[blockIdx.y]; fql_iql_prep_body(P); }

struct IqlHeadArgs {
    const float* mean;         // [B, ap]: the actor's output
    const float* log_stds;     // [act] raw, or null (const_std: 0)
    const float* act;          // [B, ap]: batch actions
    const float* eps;          // [B, ap] or null (q_actions = clip(mode))
    float *lp, *se;            // [B]: log_prob(actions); sum_j (mean - act)^2
    float* X_q;                // ddpgbc: q_actions = clip(mean + exp(ls) eps, -1, 1) into X_q[b, od + a]; else null
    int B, od, ad, ap, inp_c;
};
// The Gaussian head (distrax.MultivariateNormalDiag, temperature 1): log_prob(a) = sum_j(-((a_j - mean_j) / s_j)^2 / 2 - ls_j -
// log(2 pi) / 2), s = exp(clip(log_stds, -5, 2)).  One thread per row; accurate transcendentals.
__device__ __forceinline__ void fql_iql_head_body(const IqlHeadArgs& P) {
    const int b = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (b >= P.B) return;
    const float half_log_2pi = 0.91893853320467274f;
    const float* m = P.mean + (size_t)b * P.ap;
    const float* ac = P.act + (size_t)b * P.ap;
    float lp = 0.f, se = 0.f;
    for (int a = 0; a < P.ad; ++a) {
        const float ls = P.log_stds ? iql_clip_ls(P.log_stds[a]) : 0.0f;
        const float s = expf(ls);
        const float d = ac[a] - m[a];
        const float u = d / s;
        lp += -0.5f * u * u - ls - half_log_2pi;
        se += d * d;
        if (P.X_q) {
            const float x = P.eps ? m[a] + s * P.eps[(size_t)b * P.ap + a] : m[a];
            P.X_q[(size_t)b * P.inp_c + P.od + a] = clip1(x);
        }
    }
    P.lp[b] = lp;
    P.se[b] = se;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_head_kernel(IqlHeadArgs P) { fql_iql_head_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_head_multi_kernel(const IqlHeadArgs* __restrict__ args) { const IqlHeadArgs P = ((const FQL_CONST_AS IqlHeadArgs*)args)[blockIdx.y]; fql_iql_head_body(P); }

// dL/dlog_stds[a] = mask(raw_a) sum_b part[b, a], rows summed by thread-strided partials and a fixed block tree.  Called by the whole
// workgroup after a __syncthreads() behind the writes of `part`.
__device__ __forceinline__ void iql_reduce_log_stds(const float* part, const float* log_stds, float* g_ls, int B, int ad, int ap, float* sh) {
    for (int a = 0; a < ap; ++a) {
        float s = 0.f;
        if (a < ad)
            for (int b = threadIdx.x; b < B; b += FQL_THREADS) s += part[(size_t)b * ap + a];
        const float t = block_sum(s, sh);
        if (threadIdx.x == 0) g_ls[a] = a < ad ? iql_ls_mask(log_stds[a]) * t : 0.0f;
    }
}
__device__ __forceinline__ float iql_std_mean(const float* log_stds, int ad) {
    if (!log_stds) return 1.0f;
    float s = 0.f;
    for (int a = 0; a < ad; ++a) s += expf(iql_clip_ls(log_stds[a]));
    return s / (float)ad;
}

struct IqlAwrArgs {
    const float *qa, *qb;      // [B, 16] column 0: critic members (stored parameters) at (obs, act): the critic loss's forward pass
    const float* v;            // [B, 16] column 0: value(obs), stored parameters: the value loss's forward pass
    const float *lp, *se;      // [B]
    const float* mean;         // [B, ap]
    const float* act;          // [B, ap]
    const float* log_stds;     // [act] or null
    float* dmean;              // [B, ap]: dL/dmean for the actor's backward pass, or null (loss probe)
    float* ls_part;            // [B, ap] scratch (log_stds only)
    float* g_ls;               // [ap]: the gradient slot of log_stds, or null
    float* info;               // IQL info buffer
    int B, ad, ap;
    float alpha;
};
// agents/iql.py:59-82: adv = min(q1, q2) - v, w = min(exp(alpha adv), 100) (a constant under the gradient: every input is a stored
// parameter's), loss = -mean(w log_prob(actions)).  dL/dmean_j = -(w / B) (a_j - mean_j) / s_j^2, dL/dls_j = -(w / B) (u_j^2 - 1).
__device__ __forceinline__ void fql_iql_loss_awr_body(const IqlAwrArgs& P, float* sh) {
    float swl = 0.f, sadv = 0.f, slp = 0.f, sse = 0.f;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float adv = fminf(P.qa[(size_t)b * 16], P.qb[(size_t)b * 16]) - P.v[(size_t)b * 16];
        const float w = fminf(expf(adv * P.alpha), 100.0f);
        swl += w * P.lp[b];
        sadv += adv;
        slp += P.lp[b];
        sse += P.se[b];
    }
    const float twl = block_sum(swl, sh), tadv = block_sum(sadv, sh), tlp = block_sum(slp, sh), tse = block_sum(sse, sh);
    if (threadIdx.x == 0) {
        const float invB = 1.0f / (float)P.B;
        float* in = P.info + IQL_I_ACTOR;
        in[0] = -twl * invB;
        in[1] = tadv * invB;
        in[2] = tlp * invB;
        in[3] = tse * invB / (float)P.ad;
        in[4] = iql_std_mean(P.log_stds, P.ad);
    }
    if (!P.dmean) return;
    const float invB = 1.0f / (float)P.B;
    for (int e = threadIdx.x; e < P.B * P.ad; e += FQL_THREADS) {
        const int b = e / P.ad, a = e - b * P.ad;
        const float adv = fminf(P.qa[(size_t)b * 16], P.qb[(size_t)b * 16]) - P.v[(size_t)b * 16];
        const float w = fminf(expf(adv * P.alpha), 100.0f);
        const float s = P.log_stds ? expf(iql_clip_ls(P.log_stds[a])) : 1.0f;
        const size_t o = (size_t)b * P.ap + a;
        const float u = (P.act[o] - P.mean[o]) / s;
        P.dmean[o] = -w * invB * u / s;
        if (P.g_ls) P.ls_part[o] = -w * invB * (u * u - 1.0f);
    }
    if (!P.g_ls) return;
    __syncthreads();
    iql_reduce_log_stds(P.ls_part, P.log_stds, P.g_ls, P.B, P.ad, P.ap, sh);
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_loss_awr_kernel(IqlAwrArgs P) { __shared__ float sh[4]; fql_iql_loss_awr_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_loss_awr_multi_kernel(const IqlAwrArgs* __restrict__ args) { __shared__ float sh[4]; const IqlAwrArgs P = ((const FQL_CONST_AS IqlAwrArgs*)args)[blockIdx.y]; fql_iql_loss_awr_body(P, sh); }

struct IqlDdpgArgs {
    const float *qa, *qb;      // [B, 16] column 0: critic members (stored parameters) at (obs, q_actions)
    const float *lp, *se;      // [B]
    const float* log_stds;     // [act] or null
    float *dqa, *dqb;          // [B, 16] column 0: dL/dq seeded into the critic's input-gradient pass, or null (loss probe)
    float* info;
    int B, ad;
    float alpha;
};
// agents/iql.py:83-110: q = min(q1, q2), q_loss = -mean(q) / stop_gradient(mean |q|), bc_loss = -alpha mean(log_prob(actions)).
// dL/dq_e = -(1 / B) / mean|q| to the smaller member (1/2 each at an exact tie, as jnp.minimum's gradient).
__device__ __forceinline__ void fql_iql_loss_ddpgbc_body(const IqlDdpgArgs& P, float* sh) {
    float sq = 0.f, sa = 0.f, slp = 0.f, sse = 0.f;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float q = fminf(P.qa[(size_t)b * 16], P.qb[(size_t)b * 16]);
        sq += q;
        sa += fabsf(q);
        slp += P.lp[b];
        sse += P.se[b];
    }
    const float tq = block_sum(sq, sh), ta = block_sum(sa, sh), tlp = block_sum(slp, sh), tse = block_sum(sse, sh);
    const float invB = 1.0f / (float)P.B;
    const float qm = tq * invB, qam = ta * invB;
    if (threadIdx.x == 0) {
        const float q_loss = -qm / qam, bc_loss = -P.alpha * tlp * invB;
        float* in = P.info + IQL_I_ACTOR;
        in[0] = q_loss + bc_loss;
        in[1] = q_loss;
        in[2] = bc_loss;
        in[3] = qm;
        in[4] = qam;
        in[5] = tlp * invB;
        in[6] = tse * invB / (float)P.ad;
        in[7] = iql_std_mean(P.log_stds, P.ad);
    }
    if (!P.dqa) return;
    const float g = -invB / qam;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float a = P.qa[(size_t)b * 16], c = P.qb[(size_t)b * 16];
        const float ra = a < c ? 1.0f : (a == c ? 0.5f : 0.0f);
        P.dqa[(size_t)b * 16] = g * ra;
        P.dqb[(size_t)b * 16] = g * (1.0f - ra);
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_loss_ddpgbc_kernel(IqlDdpgArgs P) { __shared__ float sh[4]; fql_iql_loss_ddpgbc_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_loss_ddpgbc_multi_kernel(const IqlDdpgArgs* __restrict__ args) { __shared__ float sh[4]; const IqlDdpgArgs P = ((const FQL_CONST_AS IqlDdpgArgs*)args)[blockIdx.y]; fql_iql_loss_ddpgbc_body(P, sh); }

struct IqlActorGradArgs {
    const float *dxa, *dxb;    // [B, inp_c]: the critic members' input gradients (columns od .. od + ad: dL/dq_actions through q_loss)
    const float* mean;         // [B, ap]
    const float* act;          // [B, ap]
    const float* eps;          // [B, ap] or null (const_std)
    const float* log_stds;     // [act] or null
    float* dmean;              // [B, ap]
    float* ls_part;            // [B, ap] scratch (log_stds only)
    float* g_ls;               // [ap] or null
    int B, od, ad, ap, inp_c;
    float alpha;
};
// The DDPG+BC head gradient: x = mean + s eps (or mean), q_actions = clip(x, -1, 1) with mask c (1 inside, 0 outside, 1/2 at |x| = 1,
// jnp.clip); g = c dL/dq_actions.  With u = (a - mean) / s:
//   dL/dmean_j = g_j - (alpha / B) u_j / s_j,   dL/dls_j = mask(raw_j) sum_b (g_j s_j eps_j - (alpha / B) (u_j^2 - 1)).
// One workgroup: the reduction over B of the log_stds gradient runs in a fixed order.
__device__ __forceinline__ void fql_iql_actor_grad_body(const IqlActorGradArgs& P, float* sh) {
    const float ab = P.alpha / (float)P.B;
    for (int e = threadIdx.x; e < P.B * P.ad; e += FQL_THREADS) {
        const int b = e / P.ad, a = e - b * P.ad;
        const size_t o = (size_t)b * P.ap + a, oc = (size_t)b * P.inp_c + P.od + a;
        const float s = P.log_stds ? expf(iql_clip_ls(P.log_stds[a])) : 1.0f;
        const float ep = P.eps ? P.eps[o] : 0.0f;
        const float m = P.mean[o];
        const float x = P.eps ? m + s * ep : m;
        const float ax = fabsf(x);
        const float c = ax < 1.0f ? 1.0f : (ax == 1.0f ? 0.5f : 0.0f);
        const float g = c * (P.dxa[oc] + P.dxb[oc]);
        const float u = (P.act[o] - m) / s;
        P.dmean[o] = g - ab * u / s;
        if (P.g_ls) P.ls_part[o] = g * s * ep - ab * (u * u - 1.0f);
    }
    if (!P.g_ls) return;
    __syncthreads();
    iql_reduce_log_stds(P.ls_part, P.log_stds, P.g_ls, P.B, P.ad, P.ap, sh);
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_actor_grad_kernel(IqlActorGradArgs P) { __shared__ float sh[4]; fql_iql_actor_grad_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_actor_grad_multi_kernel(const IqlActorGradArgs* __restrict__ args) { __shared__ float sh[4]; const IqlActorGradArgs P = ((const FQL_CONST_AS IqlActorGradArgs*)args)[blockIdx.y]; fql_iql_actor_grad_body(P, sh); }

struct IqlFinalizeArgs {
    FinalizeArgs fin;
    float* info;       // IQL info buffer: [0, IQL_INFO_STRIDE) of an update, or the loss probe's
    int n_actor;       // IQL_N_AWR or IQL_N_DDPGBC
};
// FQL's finalize (grad statistics into DevState::info 10-12 and the step counters when do_grad_stats), then the reference's IQL order
// (fql_finalize_body declares the LDS it needs itself, sh[4] and leafn[256]: both entries get it through the inlined body)
__device__ __forceinline__ void fql_iql_finalize_body(const IqlFinalizeArgs& A) {
    fql_finalize_body(A.fin);
    if (threadIdx.x == 0) {
        const float* in = A.fin.st->info;
        float* out = A.info;
        for (int i = 0; i < 4; ++i) out[i] = in[IFQL_I_VALUE + i];
        out[4] = in[IFQL_I_CRITIC];
        for (int i = 0; i < 3; ++i) out[5 + i] = in[IFQL_I_Q + i];
        float* g = out + IQL_I_ACTOR + A.n_actor;
        for (int i = 0; i < 3; ++i) g[i] = A.fin.do_grad_stats ? in[10 + i] : 0.f;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_finalize_kernel(IqlFinalizeArgs A) { fql_iql_finalize_body(A); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_finalize_multi_kernel(const IqlFinalizeArgs* __restrict__ args) { const IqlFinalizeArgs A = ((const FQL_CONST_AS IqlFinalizeArgs*)args)[blockIdx.y]; fql_iql_finalize_body(A); }

struct IqlSampleArgs {
    const float* mean;         // [n, ap]
    const float* log_stds;     // [act] or null
    const float* eps;          // [n, ad] raw N(0, 1) or null (Philox keyed by (key, seed), rows numbered from row0)
    float* out;                // [n, ad]
    uint64_t key, seed;
    int n, ad, ap, row0;
    float temperature;
};
// agents/iql.py:158-169: clip(mean + exp(clip(log_stds)) temperature eps, -1, 1); temperature 0 is clip(mean) exactly
__device__ __forceinline__ void fql_iql_sample_body(const IqlSampleArgs& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.n * P.ad) return;
    const int r = e / P.ad, a = e - r * P.ad;
    const float m = P.mean[(size_t)r * P.ap + a];
    float x = m;
    if (P.temperature != 0.0f) {
        const float s = (P.log_stds ? expf(iql_clip_ls(P.log_stds[a])) : 1.0f) * P.temperature;
        const float ep = P.eps ? P.eps[e] : rng_normal(P.key, P.seed, 12u, (uint32_t)(P.row0 + r), (uint32_t)a);
        x = m + s * ep;
    }
    P.out[e] = clip1(x);
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_sample_kernel(IqlSampleArgs P) { fql_iql_sample_body(P); }
// (an IQL group's sampler: grid x covers the chunk's padded rows, elements past the member's n * ad return at once)
__global__ __launch_bounds__(FQL_THREADS) void fql_iql_sample_multi_kernel(const IqlSampleArgs* __restrict__ args) { const IqlSampleArgs P = ((const FQL_CONST_AS IqlSampleArgs*)args)[blockIdx.y]; fql_iql_sample_body(P); }

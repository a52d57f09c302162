// fql_rebrac.h -- the kernels of the ReBRAC agent (agents/rebrac.py) that FQL's kernels do not cover: batch assembly with next_actions,
// the deterministic actor's action (mode, target-policy noise, clips), the critic and actor losses, the gradient handed to the actor's
// backward pass and the info layout of the finalize step.  The GEMM bodies, weight gradients, LayerNorm backward, the critic's input
// gradient, Adam + Polyak and the grad statistics are FQL's.  Every reduction runs in one workgroup in a fixed order (no float atomics).
#pragma once
#include "fql_kernels.h"

// Info slots while a ReBRAC update runs: the critic loss writes 0-3, the actor loss 4-8, FQL's finalize body the grad statistics 10-12.
// fql_rebrac_finalize_kernel then moves them into the reference's order (agents/rebrac.py:48-53,78-84 + utils/flax_utils.py:151-157):
//   full step:        critic_loss, q_mean, q_max, q_min, total_loss, actor_loss, bc_loss, std, mse, grad/max, grad/min, grad/norm, 0
//   critic-only step: critic_loss, q_mean, q_max, q_min, grad/max, grad/min, grad/norm, 0, 0, 0, 0, 0, 0
enum : int { REBRAC_I_CRITIC = 0, REBRAC_I_ACTOR = 4 };

struct RebracPrepArgs {
    const SrcDesc* src;
    DevState* st;
    uint64_t key;
    int B, od, ad;
    int inp_a, inp_c, ap;   // padded input widths: actor (od), critic (od + ad); action width
    float *X_c, *X_t, *X_q; // critic inputs [B, inp_c]: [obs | act], [next_obs | .], [obs | .] (action blocks of the last two filled later)
    float *X_a, *X_ta;      // actor inputs [B, inp_a]: obs, next_obs
    float *w_act, *w_nact, *w_noise, *w_rew, *w_mask;   // [B, ap] x 3, [B] x 2
    float* gz;              // critic-only step: the actor's gradient region, zeroed here (Adam still runs over it), or null
    int64_t gz_n;
};
// utils/datasets.py:64-100 (index draw, gather, next_actions = actions[min(idx + 1, size - 1)]), agents/rebrac.py:29-33 (the raw
// N(0, 1) of the target-policy noise: Philox tensor 1, or fql_noise.eps1).  One wave per transition.
__device__ __forceinline__ void fql_rebrac_prep_body(const RebracPrepArgs& P) {
    if (P.gz)
        for (int64_t i = (int64_t)blockIdx.x * FQL_THREADS + threadIdx.x; i < P.gz_n; i += (int64_t)gridDim.x * FQL_THREADS) P.gz[i] = 0.f;
    const SrcDesc& S = *P.src;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= P.B) return;
    const uint64_t step = P.st->rng_step;
    const uint64_t key = P.key ^ (P.st->rng_stream * 0x9E3779B97F4A7C15ull);
    int64_t src = b;
    if (S.idx) src = S.idx[b];
    else if (S.use_rng_idx) src = S.lo + (int64_t)(((uint64_t)rng_u32(key, step, 7u, (uint32_t)b) * (uint64_t)S.span) >> 32);
    // dataset rows: the row after `src`, clamped to the dataset's last row (its whole size, not the shard's end); explicit batches: row b
    int64_t nrow = b;
    if (S.nact_rows > 0) nrow = src + 1 < S.nact_rows ? src + 1 : S.nact_rows - 1;
    const int od = P.od, ad = P.ad;
    const float* obs = S.obs + (size_t)src * od;
    const float* nobs = S.nobs + (size_t)src * od;
    const float* act = S.act + (size_t)src * ad;
    const float* nact = S.nact + (size_t)nrow * ad;
    const int w = P.inp_a > P.inp_c ? P.inp_a : P.inp_c;
    for (int j = lane; j < w; j += 64) {
        const bool is_obs = j < od, is_act = j >= od && j < od + ad;
        const int a = j - od;
        const float o = is_obs ? obs[j] : 0.f, no = is_obs ? nobs[j] : 0.f;
        if (j < P.inp_c) {
            const size_t r = (size_t)b * P.inp_c + j;
            P.X_c[r] = is_act ? act[a] : o;   // critic(obs, actions)  rebrac.py:44
            P.X_t[r] = no;                    // target_critic(next_obs, .)  rebrac.py:36 (action block: fql_rebrac_act_kernel)
            P.X_q[r] = o;                     // critic(obs, actor actions)  rebrac.py:61
        }
        if (j < P.inp_a) {
            P.X_a[(size_t)b * P.inp_a + j] = o;    // actor(obs)  rebrac.py:57
            P.X_ta[(size_t)b * P.inp_a + j] = no;  // target_actor(next_obs)  rebrac.py:28
        }
        if (is_act) {
            const size_t r = (size_t)b * P.ap + a;
            P.w_act[r] = act[a];
            P.w_nact[r] = nact[a];
            P.w_noise[r] = S.eps1 ? S.eps1[(size_t)b * ad + a] : rng_normal(key, step, 1u, (uint32_t)b, (uint32_t)a);
        }
    }
    if (lane == 0) {
        P.w_rew[b] = S.rew[src];
        P.w_mask[b] = S.mask[src];
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_prep_kernel(RebracPrepArgs P) { fql_rebrac_prep_body(P); }
// Multi-instance entry points (ReBRAC agent groups), here and below: blockIdx.y picks the member, its argument struct comes from a device
// array, read through the constant address space (scalar loads, as from the kernel-argument segment; fql_kernels.h FQL_CONST_AS)
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_prep_multi_kernel(const RebracPrepArgs* __restrict__ args) { const RebracPrepArgs P = ((const FQL_CONST_AS RebracPrepArgs*)args)[blockIdx.y]; fql_rebrac_prep_body(P); }

struct RebracActArgs {
    const float* mean;     // [n, ap]: mean_net output
    const float* noise;    // noise_mode 1: [n, ldn] raw N(0, 1); otherwise unused
    float* out;            // out[r * ldo + col0 + a]
    uint64_t key, seed;    // noise_mode 2: Philox keyed by (key, seed), rows numbered from row0
    int n, ad, ap, ldn, ldo, col0, row0;
    int noise_mode;        // 0: none, 1: tensor, 2: Philox
    int tanh_squash, clip_out;
    float scale, nclip;    // noise = clip(N(0, 1) * scale, +-nclip)
};
// The deterministic actor's action (utils/networks.py:82-150, const_std): mode = tanh(mean) when squashed; plus clipped noise and the
// [-1, 1] clip of the target policy (rebrac.py:28-34) and of sample_actions (rebrac.py:144-151); the actor loss's actions (rebrac.py:57-58)
// take neither.  One thread per element.
__device__ __forceinline__ void fql_rebrac_act_body(const RebracActArgs& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.n * P.ad) return;
    const int r = e / P.ad, a = e - r * P.ad;
    const float m = P.mean[(size_t)r * P.ap + a];
    float v = P.tanh_squash ? tanhf(m) : m;
    if (P.noise_mode) {
        const float z = P.noise_mode == 1 ? P.noise[(size_t)r * P.ldn + a] : rng_normal(P.key, P.seed, 11u, (uint32_t)(P.row0 + r), (uint32_t)a);
        v += fminf(fmaxf(z * P.scale, -P.nclip), P.nclip);
    }
    if (P.clip_out) v = clip1(v);
    P.out[(size_t)r * P.ldo + P.col0 + a] = v;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_act_kernel(RebracActArgs P) { fql_rebrac_act_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_act_multi_kernel(const RebracActArgs* __restrict__ args) { const RebracActArgs P = ((const FQL_CONST_AS RebracActArgs*)args)[blockIdx.y]; fql_rebrac_act_body(P); }

struct RebracCriticArgs {
    const float *qa, *qb;      // [B, 16] column 0: critic members at (obs, act)
    const float *tqa, *tqb;    // [B, 16] column 0: target critic members at (next_obs, a')
    const float* xt;           // [B, inp_c]: [next_obs | a'] (a' in columns od .. od + ad)
    const float* nact;         // [B, ap]
    const float *w_rew, *w_mask;
    float *dqa, *dqb;          // [B, 16] column 0 or null
    DevState* st;
    int B, od, ad, inp_c, ap;
    float discount, alpha_critic;
};
// rebrac.py:36-53: next_q = min(target q1, q2) - alpha_critic sum((a' - next_actions)^2); y = r + discount mask next_q;
// loss = mean over (2, B) of (q - y)^2; q_mean / q_max / q_min over all 2B values of q
__device__ __forceinline__ void fql_rebrac_loss_critic_body(const RebracCriticArgs& P, float* sh) {
    const float gs = 1.0f / (float)P.B;   // d/dq of mean over 2B of (q - y)^2
    float sl = 0.f, sq = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        float pen = 0.f;
        for (int a = 0; a < P.ad; ++a) {
            const float d = P.xt[(size_t)b * P.inp_c + P.od + a] - P.nact[(size_t)b * P.ap + a];
            pen += d * d;
        }
        const float nq = fminf(P.tqa[(size_t)b * 16], P.tqb[(size_t)b * 16]) - P.alpha_critic * pen;
        const float y = P.w_rew[b] + P.discount * P.w_mask[b] * nq;
        const float qa = P.qa[(size_t)b * 16], qb = P.qb[(size_t)b * 16];
        const float da = qa - y, db = qb - y;
        sl += da * da + db * db;
        sq += qa + qb;
        mx = fmaxf(mx, fmaxf(qa, qb));
        mn = fminf(mn, fminf(qa, qb));
        if (P.dqa) {
            P.dqa[(size_t)b * 16] = gs * da;
            P.dqb[(size_t)b * 16] = gs * db;
        }
    }
    const float tl = block_sum(sl, sh), tq = block_sum(sq, sh);
    const float tmx = block_max(mx, sh), tmn = -block_max(-mn, sh);
    if (threadIdx.x == 0) {
        const float inv = 1.0f / (2.0f * (float)P.B);
        float* in = P.st->info + REBRAC_I_CRITIC;
        in[0] = tl * inv;
        in[1] = tq * inv;
        in[2] = tmx;
        in[3] = tmn;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_loss_critic_kernel(RebracCriticArgs P) { __shared__ float sh[4]; fql_rebrac_loss_critic_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_loss_critic_multi_kernel(const RebracCriticArgs* __restrict__ args) { __shared__ float sh[4]; const RebracCriticArgs P = ((const FQL_CONST_AS RebracCriticArgs*)args)[blockIdx.y]; fql_rebrac_loss_critic_body(P, sh); }

struct RebracActorArgs {
    const float *qa, *qb;      // [B, 16] column 0: critic members (stored parameters) at (obs, a)
    const float* xq;           // [B, inp_c]: [obs | a]
    const float* act;          // [B, ap]: the batch's actions
    float *dqa, *dqb;          // [B, 16] column 0: dL/dq seeded into the critic's input-gradient pass, or null
    DevState* st;
    int B, od, ad, inp_c, ap;
    float alpha_actor;
};
// rebrac.py:55-84: q = min(q1, q2), lam = 1 / mean|q| (no gradient), actor_loss = -mean(lam q), bc_loss = alpha_actor mean(sum((a - act)^2)),
// std = 1 (const_std: log_std 0, temperature 1).  At a tie the gradient of min splits equally between the members, as jnp.min's does.
__device__ __forceinline__ void fql_rebrac_loss_actor_body(const RebracActorArgs& P, float* sh) {
    float s = 0.f, sa = 0.f, se = 0.f;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float q = fminf(P.qa[(size_t)b * 16], P.qb[(size_t)b * 16]);
        s += q;
        sa += fabsf(q);
        float m = 0.f;
        for (int a = 0; a < P.ad; ++a) {
            const float d = P.xq[(size_t)b * P.inp_c + P.od + a] - P.act[(size_t)b * P.ap + a];
            m += d * d;
        }
        se += m;
    }
    const float ts = block_sum(s, sh), tsa = block_sum(sa, sh), tse = block_sum(se, sh);
    const float invB = 1.0f / (float)P.B;
    const float lam = 1.0f / (tsa * invB);
    if (P.dqa) {
        const float g = -lam * invB;
        for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
            const float qa = P.qa[(size_t)b * 16], qb = P.qb[(size_t)b * 16];
            P.dqa[(size_t)b * 16] = qa < qb ? g : (qa == qb ? 0.5f * g : 0.f);
            P.dqb[(size_t)b * 16] = qb < qa ? g : (qa == qb ? 0.5f * g : 0.f);
        }
    }
    if (threadIdx.x == 0) {
        const float actor = -(lam * (ts * invB)), mse = tse * invB, bc = P.alpha_actor * mse;
        float* in = P.st->info + REBRAC_I_ACTOR;
        in[0] = actor + bc;
        in[1] = actor;
        in[2] = bc;
        in[3] = 1.0f;
        in[4] = mse;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_loss_actor_kernel(RebracActorArgs P) { __shared__ float sh[4]; fql_rebrac_loss_actor_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_loss_actor_multi_kernel(const RebracActorArgs* __restrict__ args) { __shared__ float sh[4]; const RebracActorArgs P = ((const FQL_CONST_AS RebracActorArgs*)args)[blockIdx.y]; fql_rebrac_loss_actor_body(P, sh); }

struct RebracActorGradArgs {
    const float *dxa, *dxb;    // [B, inp_c]: the critic members' input gradients (columns od .. od + ad: dL/da through the Q term)
    const float* xq;           // [B, inp_c]: [obs | a]
    const float* act;          // [B, ap]
    float* dmean;              // [B, ap]: dL/dmean for the actor's backward pass
    int B, od, ad, inp_c, ap;
    float gbc;                 // alpha_actor 2 / B
    int tanh_squash;
};
// dL/da = dQ-term/da + alpha_actor 2 (a - act) / B; through the tanh of the mode: dL/dmean = dL/da (1 - a^2)
__device__ __forceinline__ void fql_rebrac_actor_grad_body(const RebracActorGradArgs& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.B * P.ad) return;
    const int b = e / P.ad, a = e - b * P.ad;
    const size_t o = (size_t)b * P.inp_c + P.od + a;
    const float av = P.xq[o];
    float g = P.dxa[o] + P.dxb[o] + P.gbc * (av - P.act[(size_t)b * P.ap + a]);
    if (P.tanh_squash) g *= 1.0f - av * av;
    P.dmean[(size_t)b * P.ap + a] = g;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_actor_grad_kernel(RebracActorGradArgs P) { fql_rebrac_actor_grad_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_actor_grad_multi_kernel(const RebracActorGradArgs* __restrict__ args) { const RebracActorGradArgs P = ((const FQL_CONST_AS RebracActorGradArgs*)args)[blockIdx.y]; fql_rebrac_actor_grad_body(P); }

// FQL's finalize (grad statistics into slots 10-12 and the step counters), then the reference's ReBRAC order for the step's kind
__device__ __forceinline__ void fql_rebrac_finalize_body(const FinalizeArgs& A, int full) {
    fql_finalize_body(A);
    if (threadIdx.x == 0 && A.do_grad_stats) {
        float* in = A.st->info;
        const float gmax = in[10], gmin = in[11], gn = in[12];
        const int g0 = full ? 9 : 4;
        in[g0] = gmax; in[g0 + 1] = gmin; in[g0 + 2] = gn;
        for (int i = g0 + 3; i < 13; ++i) in[i] = 0.f;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_finalize_kernel(FinalizeArgs A, int full) { fql_rebrac_finalize_body(A, full); }
// The two arguments of the kernel above as one struct, laid out as its kernel-argument segment lays them out (A at 0, full behind it), so
// that the bytes a member's launch binds are a prefix of its element of the multi-instance kernel's array
struct RebracFinalizeArgs {
    FinalizeArgs A;
    int full;
};
static_assert(offsetof(RebracFinalizeArgs, full) == sizeof(FinalizeArgs) && alignof(FinalizeArgs) >= alignof(int), "RebracFinalizeArgs must match the (FinalizeArgs, int) kernel-argument layout");
__global__ __launch_bounds__(FQL_THREADS) void fql_rebrac_finalize_multi_kernel(const RebracFinalizeArgs* __restrict__ args) { const RebracFinalizeArgs R = ((const FQL_CONST_AS RebracFinalizeArgs*)args)[blockIdx.y]; fql_rebrac_finalize_body(R.A, R.full); }

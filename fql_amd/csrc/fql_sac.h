// fql_sac.h -- the kernels of the SAC agent (agents/sac.py; RLPD is this agent run online with balanced sampling) that FQL's kernels do
// not cover: batch assembly with the two Gaussian noise tensors, the squashed Gaussian actor's sample and log-probability, the critic and
// actor losses (with the temperature's own loss and gradient), the gradient handed to the actor's two heads and the info layout of the
// finalize step.  The GEMM bodies, weight gradients, LayerNorm backward, the critic's input gradient, Adam + Polyak and the grad
// statistics are FQL's.  Every reduction runs in one workgroup in a fixed order (no float atomics).
// Every kernel a SAC agent group fuses (fql_sac_group_*) comes in three parts: a __device__ body, the by-value
// entry a single handle launches, and a *_multi_kernel that takes a device array of the same argument struct, one per member.
//
// The actor's two heads (mean_net, log_std_net) are one [H, 2 ap] layer of the arena: columns [0, ap) the mean, [ap, 2 ap) the raw
// log-std (the leaves read back as separate [H, act] / [act] arrays, build_leaves()).
#pragma once
#include "fql_kernels.h"

// Info slots while a SAC update runs: the critic loss writes 0-3, the actor loss 4-9 and actor/q into scratch slot 14;
// fql_sac_finalize_kernel then writes the reference's order (agents/sac.py:51-56,84-92 +
// utils/flax_utils.py:151-157): critic_loss, q_mean, q_max, q_min, total_loss, actor_loss, alpha_loss, alpha, entropy, std, q,
// grad/max, grad/min, grad/norm.
enum : int { SAC_I_CRITIC = 0, SAC_I_ACTOR = 4, SAC_I_Q = 14 };
#define SAC_LOG_STD_MIN (-5.0f)
#define SAC_LOG_STD_MAX 2.0f

struct SacPrepArgs {
    const SrcDesc* src;
    DevState* st;
    uint64_t key;
    int B, od, ad;
    int inp_a, inp_c, ap;   // padded input widths: actor (od), critic (od + ad); action width
    float *X_c, *X_t, *X_q; // critic inputs [B, inp_c]: [obs | act], [next_obs | .], [obs | .] (action blocks of the last two filled later)
    float* X_a;             // actor input [2B, inp_a]: obs rows, then next_obs rows
    float* w_eps;           // [2B, ap]: eps_c (the actor loss's noise) rows, then eps_n (the critic loss's next-action noise) rows
    float *w_rew, *w_mask;  // [B] x 2
};
// utils/datasets.py:64-100 (index draw and gather, from one source or the two of a balanced batch, main.py:255-259) and the raw N(0, 1) of
// the two samples (agents/sac.py:27,62): eps_n = fql_noise.eps1 or Philox tensor 1, eps_c = fql_noise.eps2 or Philox tensor 5.  One wave
// per transition.
__device__ __forceinline__ void fql_sac_prep_body(const SacPrepArgs P) {
    const SrcDesc& S = *P.src;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= P.B) return;
    const uint64_t step = P.st->rng_step;
    const uint64_t key = P.key ^ (P.st->rng_stream * 0x9E3779B97F4A7C15ull);
    int64_t src = b;
    const bool second = S.split > 0 && b >= S.split;   // the replay half of a balanced batch
    if (S.idx) src = S.idx[b];
    else if (S.use_rng_idx) {
        const uint64_t u = rng_u32(key, step, 7u, (uint32_t)b);
        src = second ? S.lo2 + (int64_t)((u * (uint64_t)S.span2) >> 32) : S.lo + (int64_t)((u * (uint64_t)S.span) >> 32);
    }
    const int od = P.od, ad = P.ad;
    const float* obs = (second ? S.obs2 : S.obs) + (size_t)src * od;
    const float* nobs = (second ? S.nobs2 : S.nobs) + (size_t)src * od;
    const float* act = (second ? S.act2 : S.act) + (size_t)src * ad;
    const int w = P.inp_a > P.inp_c ? P.inp_a : P.inp_c;
    for (int j = lane; j < w; j += 64) {
        const bool is_obs = j < od, is_act = j >= od && j < od + ad;
        const int a = j - od;
        const float o = is_obs ? obs[j] : 0.f, no = is_obs ? nobs[j] : 0.f;
        if (j < P.inp_c) {
            const size_t r = (size_t)b * P.inp_c + j;
            P.X_c[r] = is_act ? act[a] : o;   // critic(obs, actions)  sac.py:46
            P.X_t[r] = no;                    // target_critic(next_obs, .)  sac.py:30 (action block: fql_sac_act_kernel)
            P.X_q[r] = o;                     // critic(obs, actor actions)  sac.py:63 (action block: fql_sac_act_kernel)
        }
        if (j < P.inp_a) {
            P.X_a[(size_t)b * P.inp_a + j] = o;              // actor(obs)  sac.py:61
            P.X_a[(size_t)(P.B + b) * P.inp_a + j] = no;     // actor(next_obs)  sac.py:26
        }
        if (is_act) {
            P.w_eps[(size_t)b * P.ap + a] = S.eps2 ? S.eps2[(size_t)b * ad + a] : rng_normal(key, step, 5u, (uint32_t)b, (uint32_t)a);
            P.w_eps[(size_t)(P.B + b) * P.ap + a] = S.eps1 ? S.eps1[(size_t)b * ad + a] : rng_normal(key, step, 1u, (uint32_t)b, (uint32_t)a);
        }
    }
    if (lane == 0) {
        P.w_rew[b] = (second ? S.rew2 : S.rew)[src];
        P.w_mask[b] = (second ? S.mask2 : S.mask)[src];
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_prep_kernel(SacPrepArgs P) { fql_sac_prep_body(P); }
// Multi-instance entry points (SAC agent groups), here and below: blockIdx.y picks the member, its argument struct comes from a device
// array, read through the constant address space (scalar loads, as from the kernel-argument segment; fql_kernels.h FQL_CONST_AS).
// Shared-memory arrays are declared in the entries and handed to the body: the single-workgroup kernels run as grid (1, members), each
// workgroup the member's own fixed-order reduction.  Grid x = rows / 4.
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_prep_multi_kernel(const SacPrepArgs* __restrict__ args) { const SacPrepArgs P = ((const FQL_CONST_AS SacPrepArgs*)args)[blockIdx.y]; fql_sac_prep_body(P); }

// softplus(y) = log(1 + e^y) without overflow for large |y|
__device__ __forceinline__ float sac_softplus(float y) { return fmaxf(y, 0.0f) + log1pf(expf(-fabsf(y))); }

struct SacActArgs {
    const float* head;     // [n, 2 ap]: mean (columns 0 .. ad - 1), raw log-std (columns ap .. ap + ad - 1)
    const float* eps;      // noise_mode 1: [n, lde] raw N(0, 1); otherwise unused
    float* out;            // rows r < nsplit: out[r * ldo + col0 + a]
    float* out2;           // rows r >= nsplit: out2[(r - nsplit) * ldo + col0 + a]
    float* lp;             // [n] log-probabilities of the samples, or null
    uint64_t key, seed;    // noise_mode 2: Philox keyed by (key, seed), rows numbered from row0
    int n, ad, ap, lde, ldo, col0, row0, nsplit;
    int noise_mode;        // 1: tensor, 2: Philox
    int tanh_squash, clip_out;
    float temperature;
};
// The squashed Gaussian actor (utils/networks.py:118-150, state-dependent std): ls = clip(log_std_net(h), -5, 2), x = mean + exp(ls)
// temperature eps, a = tanh(x) (or x); distrax's sample_and_log_prob: log_prob = sum_j (-eps_j^2 / 2 - log(exp(ls_j) temperature) -
// log(2 pi) / 2) - [tanh] sum_j 2 (log 2 - x_j - softplus(-2 x_j)).  sample_actions (sac.py:136-149) adds the [-1, 1] clip.  One thread
// per row; accurate transcendentals.
__device__ __forceinline__ void fql_sac_act_body(const SacActArgs& P) {
    const int r = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (r >= P.n) return;
    const float* h = P.head + (size_t)r * 2 * P.ap;
    float* o = r < P.nsplit ? P.out + (size_t)r * P.ldo + P.col0 : P.out2 + (size_t)(r - P.nsplit) * P.ldo + P.col0;
    const float half_log_2pi = 0.91893853320467274f, log2 = 0.69314718055994531f;
    float lp = 0.f;
    for (int a = 0; a < P.ad; ++a) {
        const float ls = fminf(fmaxf(h[P.ap + a], SAC_LOG_STD_MIN), SAC_LOG_STD_MAX);
        const float sc = expf(ls) * P.temperature;
        const float e = P.noise_mode == 1 ? P.eps[(size_t)r * P.lde + a] : rng_normal(P.key, P.seed, 11u, (uint32_t)(P.row0 + r), (uint32_t)a);
        const float x = h[a] + sc * e;
        lp += -0.5f * e * e - ls - logf(P.temperature) - half_log_2pi;
        float v = x;
        if (P.tanh_squash) {
            lp -= 2.0f * (log2 - x - sac_softplus(-2.0f * x));
            v = tanhf(x);
        }
        if (P.clip_out) v = clip1(v);
        o[a] = v;
    }
    if (P.lp) P.lp[r] = lp;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_act_kernel(SacActArgs P) { fql_sac_act_body(P); }
// (a SAC group's sampler binds this one too: grid x covers the chunk's padded rows, rows past the member's n return at once)
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_act_multi_kernel(const SacActArgs* __restrict__ args) { const SacActArgs P = ((const FQL_CONST_AS SacActArgs*)args)[blockIdx.y]; fql_sac_act_body(P); }

struct SacCriticArgs {
    const float *qa, *qb;      // [B, 16] column 0: critic members at (obs, act)
    const float *tqa, *tqb;    // [B, 16] column 0: target critic members at (next_obs, a')
    const float* lpn;          // [B]: log_prob(a')
    const float *w_rew, *w_mask;
    const float* log_alpha;    // the arena's modules_alpha/log_value (stored parameter)
    float *dqa, *dqb;          // [B, 16] column 0 or null
    DevState* st;
    int B, q_min, backup_entropy;
    float discount;
};
// sac.py:23-56: next_q = min (or mean) of the target pair; y = r + discount mask next_q (- discount mask lp' alpha with backup_entropy);
// loss = mean over (2, B) of (q - y)^2; q_mean / q_max / q_min over all 2B values of q
__device__ __forceinline__ void fql_sac_loss_critic_body(const SacCriticArgs& P, float* sh) {
    const float gs = 1.0f / (float)P.B;   // d/dq of mean over 2B of (q - y)^2
    const float alpha = expf(P.log_alpha[0]);
    float sl = 0.f, sq = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float ta = P.tqa[(size_t)b * 16], tb = P.tqb[(size_t)b * 16];
        const float nq = P.q_min ? fminf(ta, tb) : 0.5f * (ta + tb);
        float y = P.w_rew[b] + P.discount * P.w_mask[b] * nq;
        if (P.backup_entropy) y -= P.discount * P.w_mask[b] * P.lpn[b] * alpha;
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
        float* in = P.st->info + SAC_I_CRITIC;
        in[0] = tl * inv;
        in[1] = tq * inv;
        in[2] = tmx;
        in[3] = tmn;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_loss_critic_kernel(SacCriticArgs P) { __shared__ float sh[4]; fql_sac_loss_critic_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_loss_critic_multi_kernel(const SacCriticArgs* __restrict__ args) { __shared__ float sh[4]; const SacCriticArgs P = ((const FQL_CONST_AS SacCriticArgs*)args)[blockIdx.y]; fql_sac_loss_critic_body(P, sh); }

struct SacActorArgs {
    const float *qa, *qb;      // [B, 16] column 0: critic members (stored parameters) at (obs, a)
    const float* lp;           // [B]: log_prob(a)
    const float* head;         // [B, 2 ap]: the actor's head outputs on the obs rows
    const float* log_alpha;    // stored modules_alpha/log_value
    float* g_log_alpha;        // its gradient slot, or null (loss probe)
    float *dqa, *dqb;          // [B, 16] column 0: dL/dq seeded into the critic's input-gradient pass, or null
    DevState* st;
    int B, ad, ap;
    float target_entropy;
};
// sac.py:58-92: qbar = mean of the pair, actor_loss = mean(alpha lp - qbar) (alpha held constant), entropy = -mean(lp),
// alpha_loss = alpha (entropy - target_entropy) with d/dlog_value = alpha (entropy - target_entropy), std = mean of exp(ls) over [B, act]
__device__ __forceinline__ void fql_sac_loss_actor_body(const SacActorArgs& P, float* sh) {
    float slp = 0.f, sq = 0.f, ss = 0.f;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        slp += P.lp[b];
        sq += 0.5f * (P.qa[(size_t)b * 16] + P.qb[(size_t)b * 16]);
        const float* h = P.head + (size_t)b * 2 * P.ap + P.ap;
        for (int a = 0; a < P.ad; ++a) ss += expf(fminf(fmaxf(h[a], SAC_LOG_STD_MIN), SAC_LOG_STD_MAX));
        if (P.dqa) {
            const float g = -0.5f / (float)P.B;
            P.dqa[(size_t)b * 16] = g;
            P.dqb[(size_t)b * 16] = g;
        }
    }
    const float tlp = block_sum(slp, sh), tq = block_sum(sq, sh), ts = block_sum(ss, sh);
    if (threadIdx.x == 0) {
        const float invB = 1.0f / (float)P.B;
        const float alpha = expf(P.log_alpha[0]);
        const float mlp = tlp * invB, q = tq * invB;
        const float actor = alpha * mlp - q, entropy = -mlp;
        const float alpha_loss = alpha * (entropy - P.target_entropy);
        if (P.g_log_alpha) P.g_log_alpha[0] = alpha_loss;
        float* in = P.st->info;
        in[SAC_I_ACTOR + 0] = actor + alpha_loss;
        in[SAC_I_ACTOR + 1] = actor;
        in[SAC_I_ACTOR + 2] = alpha_loss;
        in[SAC_I_ACTOR + 3] = alpha;
        in[SAC_I_ACTOR + 4] = entropy;
        in[SAC_I_ACTOR + 5] = ts / ((float)P.B * (float)P.ad);
        in[SAC_I_Q] = q;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_loss_actor_kernel(SacActorArgs P) { __shared__ float sh[4]; fql_sac_loss_actor_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_loss_actor_multi_kernel(const SacActorArgs* __restrict__ args) { __shared__ float sh[4]; const SacActorArgs P = ((const FQL_CONST_AS SacActorArgs*)args)[blockIdx.y]; fql_sac_loss_actor_body(P, sh); }

struct SacActorGradArgs {
    const float *dxa, *dxb;    // [B, inp_c]: the critic members' input gradients (columns od .. od + ad: dL/da through the Q term)
    const float* xq;           // [B, inp_c]: [obs | a]
    const float* head;         // [B, 2 ap]: mean, raw log-std
    const float* eps;          // [B, ap]: eps_c
    const float* log_alpha;
    float* dhead;              // [B, 2 ap]: dL/dmean, dL/dlog_std_raw for the actor's backward pass
    int B, od, ad, inp_c, ap;
    int tanh_squash;
};
// Through sample_and_log_prob (x = mean + s eps, the Gaussian term of lp depends on mean only through x and cancels):
//   g_x = alpha 2 a / B + (1 - a^2) dL_Q/da with tanh, dL_Q/da without; dL/dmean = g_x;
//   dL/dls_raw = clipmask (g_x s eps - alpha / B), clipmask 1 inside (-5, 2), 0 outside, 1/2 at a bound (jnp.clip's max / min).
// (the body takes the struct by value: through a reference the by-value entry compiles to 17 VGPRs and 1028 bytes, this way to the 16
// and 956 it had as one function)
__device__ __forceinline__ void fql_sac_actor_grad_body(const SacActorGradArgs P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.B * P.ad) return;
    const int b = e / P.ad, a = e - b * P.ad;
    const size_t o = (size_t)b * P.inp_c + P.od + a;
    const float invB = 1.0f / (float)P.B;
    const float alpha = expf(P.log_alpha[0]);
    const float av = P.xq[o];
    const float dq = P.dxa[o] + P.dxb[o];
    const float gx = P.tanh_squash ? alpha * 2.0f * av * invB + (1.0f - av * av) * dq : dq;
    const float raw = P.head[(size_t)b * 2 * P.ap + P.ap + a];
    const float ls = fminf(fmaxf(raw, SAC_LOG_STD_MIN), SAC_LOG_STD_MAX);
    const float cm = (raw > SAC_LOG_STD_MIN && raw < SAC_LOG_STD_MAX) ? 1.0f : ((raw == SAC_LOG_STD_MIN || raw == SAC_LOG_STD_MAX) ? 0.5f : 0.0f);
    const float s = expf(ls);
    float* d = P.dhead + (size_t)b * 2 * P.ap;
    d[a] = gx;
    d[P.ap + a] = cm * (gx * s * P.eps[(size_t)b * P.ap + a] - alpha * invB);
}
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_actor_grad_kernel(SacActorGradArgs P) { fql_sac_actor_grad_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_actor_grad_multi_kernel(const SacActorGradArgs* __restrict__ args) { const SacActorGradArgs P = ((const FQL_CONST_AS SacActorGradArgs*)args)[blockIdx.y]; fql_sac_actor_grad_body(P); }

// FQL's finalize (grad statistics, then the step counters) with one change: a leaf's chunk partials are folded by a whole wave (lane-strided
// sums, then a fixed xor tree), not by 4 threads.  SAC's head leaves have one Adam chunk per padded row (build_leaves: 2 x H chunks), which
// FQL's 4-threads-per-leaf loop walks sequentially on the update's serial tail (14.5 us per update at H = 512, against 5.7 us for FQL's
// finalize).  Fixed order throughout: bitwise reproducible.  Then the reference's SAC order (14 infos).
__device__ __forceinline__ void fql_sac_finalize_body(const FinalizeArgs& A, float* sh, float* leafn) {
    DevState* st = A.st;
    tl_enter(A.tl);
    if (!A.do_grad_stats) return;
    float mx = -INFINITY, mn = INFINITY;
    for (int cidx = threadIdx.x; cidx < A.n_chunks; cidx += FQL_THREADS) {
        mx = fmaxf(mx, A.partials[4 * cidx + 1]);
        mn = fminf(mn, A.partials[4 * cidx + 2]);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int l = wave; l < A.nleaves; l += FQL_THREADS / 64) {
        const int b = A.leaf_range[l], e = A.leaf_range[l + 1];
        float s = 0.f;
        for (int cidx = b + lane; cidx < e; cidx += 64) s += A.partials[4 * cidx];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) leafn[l] = sqrtf(s);
    }
    const float tmx = block_max(mx, sh), tmn = -block_max(-mn, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
        float nrm = 0.f;
        for (int i = 0; i < A.nleaves; ++i) nrm += leafn[i];
        float* in = st->info;
        in[10] = in[SAC_I_Q];
        in[11] = fmaxf(tmx, 0.0f);
        in[12] = fminf(tmn, 0.0f);
        in[13] = nrm;
        st->rng_step += 1;
        st->adam_count += 1;
        st->train_step += 1;
        st->b1pow *= 0.9;
        st->b2pow *= 0.999;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_finalize_kernel(FinalizeArgs A) { __shared__ float sh[4]; __shared__ float leafn[256]; fql_sac_finalize_body(A, sh, leafn); }
__global__ __launch_bounds__(FQL_THREADS) void fql_sac_finalize_multi_kernel(const FinalizeArgs* __restrict__ args) { __shared__ float sh[4]; __shared__ float leafn[256]; const FinalizeArgs A = ((const FQL_CONST_AS FinalizeArgs*)args)[blockIdx.y]; fql_sac_finalize_body(A, sh, leafn); }

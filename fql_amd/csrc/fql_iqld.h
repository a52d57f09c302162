// fql_iqld.h -- the kernels of the IQL-diffusion agent (agents/iql_diffusion.py, the binary optimality family) that the other headers
// do not cover: batch assembly with the two embedding rows, the critic loss at the reference's 1 / (2B) scaling with member 0's mean,
// the loss weights and their statistics, the weighted two-half flow-matching loss, the embedding gradient, the per-TrainState finalize
// and the sampler's step-bias table, layer 0 and classifier-free-guidance step.  The value loss is IFQL's (fql_ifql_loss_value_kernel);
// the GEMM bodies, weight gradients, LayerNorm backward, Adam + Polyak and the sampler's row assembly (fql_bc_assemble_kernel) are
// FQL's and BC's.  Every reduction runs in one workgroup in a fixed order (no float atomics).  At the end of the file: the two kernels
// of the sweep programs (one guidance weight per row), the guidance step folded into the next step's layer 0 and the last step alone.
// Every kernel an IQL-diffusion agent group fuses (fql_iqld_group_*) comes in three parts: a __device__ body, the
// by-value entry a single handle launches, and a *_multi_kernel that takes a device array of the same argument struct, one per member.
//
// The actor (DiffusionPolicy) is MLP(hidden, GELU, LayerNorm) + Dense(act) on [obs | x_t | emb(t) | Embed[is_positive]]: BC's policy
// with 32 more input columns.  The positive and the unconditional pass of a batch share obs, x_t, t and vel, so they run as ONE pass
// over 2B rows: rows [0, B) carry Embed[1], rows [B, 2B) carry Embed[0].
#pragma once
#include "fql_bc.h"
#include "fql_ifql.h"

enum : int { IQLD_EMBED = 32, IQLD_NUM_INFO = 21, IQLD_INFO_STRIDE = 32 };
// The infos, in the order of fql_handle_info_name (agents/iql_diffusion.py:94-116,197-213 + utils/flax_utils.py:151-157):
//   0 critic_loss 1 q | 2 value_loss 3 v 4 v_min 5 v_max | 6 actor_q 7 actor_loss 8 actor_positive_ratio 9 actor_loss_positive
//   10 actor_loss_uncond 11 o_mean 12 o_std 13 o_min 14 o_max 15 effective_batch_size 16 loss_weights_top_10_mass 17 loss_weights_max |
//   18 grad/max 19 grad/min 20 grad/norm
enum : int { IQLD_I_CRITIC = 0, IQLD_I_VALUE = 2, IQLD_I_ACTOR = 6, IQLD_I_GRAD = 18 };
enum : int { IQLD_BINARY = 0, IQLD_BINARY_AWR = 1, IQLD_BINARY_SOFTMAX = 2 };
enum : int { IQLD_ROWS_LOSSES = 0, IQLD_ROWS_O = 1, IQLD_ROWS_WEIGHTS = 2 };

struct IqldPrepArgs {
    const SrcDesc* src;
    DevState* st;
    uint64_t key;
    const float* emb;          // [(S + 1), 16] timestep-embedding table
    const float* embed;        // [2, 32]: Embed_0/embedding of the current parameters
    int B, od, ad;
    int inp_v, inp_c, inp_b, ap, S;   // padded input widths: value (od), critic (od + ad), actor (od + ad + 16 + 32); action width; denoise_steps
    float *X_v, *X_c, *X_bc, *vel, *w_rew, *w_mask;   // [2B, inp_v], [B, inp_c], [2B, inp_b], [B, ap], [B], [B]
};
// utils/datasets.py:64-100 (index draw + gather), agents/iql_diffusion.py:172-186 (x_0, k, x_t, vel and the two actor inputs): one wave
// per transition.  x_0 is Philox tensor 2 and k = floor(u32 (S + 1) / 2^32) of tensor 3, as BC's; explicit tensors replace them.
__device__ __forceinline__ void fql_iqld_prep_body(const IqldPrepArgs& P) {
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
    int k = S.t ? (int)rintf(S.t[b] * (float)P.S) : (int)(((uint64_t)rng_u32(key, step, 3u, (uint32_t)b) * (uint64_t)(P.S + 1)) >> 32);
    k = k < 0 ? 0 : (k > P.S ? P.S : k);
    const float tt = (float)k / (float)P.S;
    const float* em = P.emb + (size_t)k * BC_EMB;
    int w = P.inp_v > P.inp_c ? P.inp_v : P.inp_c;
    w = w > P.inp_b ? w : P.inp_b;
    const int e0 = od + ad, e1 = e0 + BC_EMB, e2 = e1 + IQLD_EMBED;
    for (int j = lane; j < w; j += 64) {
        const bool is_obs = j < od, is_act = j >= od && j < e0;
        const int a = j - od;
        const float o = is_obs ? obs[j] : 0.f;
        float av = 0.f, xx = 0.f;
        if (is_act) {
            av = act[a];
            xx = S.x0 ? S.x0[(size_t)b * ad + a] : rng_normal(key, step, 2u, (uint32_t)b, (uint32_t)a);
        }
        if (j < P.inp_v) {
            P.X_v[(size_t)b * P.inp_v + j] = o;                               // value(obs)       iql_diffusion.py:109,131
            P.X_v[(size_t)(B + b) * P.inp_v + j] = is_obs ? nobs[j] : 0.f;    // value(next_obs)  iql_diffusion.py:96
        }
        if (j < P.inp_c) P.X_c[(size_t)b * P.inp_c + j] = is_act ? av : o;    // (target_)critic(obs, actions)  iql_diffusion.py:98,107,133-135
        if (j < P.inp_b) {
            float pos = 0.f, unc = 0.f;
            if (is_obs) pos = unc = o;
            else if (is_act) pos = unc = (1.0f - tt) * xx + tt * av;          // iql_diffusion.py:177
            else if (j < e1) pos = unc = em[j - e0];
            else if (j < e2) { pos = P.embed[IQLD_EMBED + (j - e1)]; unc = P.embed[j - e1]; }
            P.X_bc[(size_t)b * P.inp_b + j] = pos;                            // actor(obs, o = 1, x_t, t)  iql_diffusion.py:181
            P.X_bc[(size_t)(B + b) * P.inp_b + j] = unc;                      // actor(obs, 0, x_t, t)      iql_diffusion.py:186
        }
        if (is_act) P.vel[(size_t)b * P.ap + a] = av - xx;                    // iql_diffusion.py:178
    }
    if (lane == 0) {
        P.w_rew[b] = S.rew[src];
        P.w_mask[b] = S.mask[src];
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_prep_kernel(IqldPrepArgs P) { fql_iqld_prep_body(P); }
// Multi-instance entry points (IQL-diffusion agent groups), here and below: blockIdx.y picks the member, its argument struct comes from a
// device array, read through the constant address space (scalar loads, as from the kernel-argument segment; fql_kernels.h FQL_CONST_AS).
// Shared-memory arrays are declared in the entries and handed to the body.
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_prep_multi_kernel(const IqldPrepArgs* __restrict__ args) { const IqldPrepArgs P = ((const FQL_CONST_AS IqldPrepArgs*)args)[blockIdx.y]; fql_iqld_prep_body(P); }

struct IqldCriticArgs {
    const float* nv;           // [B, 16] column 0: value(next_obs), stored parameters (rows B..2B-1 of the value pass)
    const float *qa, *qb;      // [B, 16] column 0: critic members at (obs, act)
    const float *w_rew, *w_mask;
    float *dqa, *dqb;          // [B, 16] column 0 or null
    float* info;               // the handle's info buffer (update or probe half)
    int B;
    float discount;
};
// agents/iql_diffusion.py:94-103: y = r + discount mask v(next_obs); loss = mean over BOTH members and the batch of (q_e - y)^2, i.e.
// 1 / (2B) where agents/iql.py sums the members; q = mean of member 0
__device__ __forceinline__ void fql_iqld_loss_critic_body(const IqldCriticArgs& P, float* sh) {
    const float gs = 1.0f / (float)P.B;   // 2 / (2B)
    float sl = 0.f, sq = 0.f;
    for (int b = threadIdx.x; b < P.B; b += FQL_THREADS) {
        const float y = P.w_rew[b] + P.discount * P.w_mask[b] * P.nv[(size_t)b * 16];
        const float qa = P.qa[(size_t)b * 16];
        const float da = qa - y, db = P.qb[(size_t)b * 16] - y;
        sl += da * da + db * db;
        sq += qa;
        if (P.dqa) {
            P.dqa[(size_t)b * 16] = gs * da;
            P.dqb[(size_t)b * 16] = gs * db;
        }
    }
    const float tl = block_sum(sl, sh), tq = block_sum(sq, sh);
    if (threadIdx.x == 0) {
        P.info[IQLD_I_CRITIC] = tl / (2.0f * (float)P.B);
        P.info[IQLD_I_CRITIC + 1] = tq / (float)P.B;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_loss_critic_kernel(IqldCriticArgs P) { __shared__ float sh[4]; fql_iqld_loss_critic_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_loss_critic_multi_kernel(const IqldCriticArgs* __restrict__ args) { __shared__ float sh[4]; const IqldCriticArgs P = ((const FQL_CONST_AS IqldCriticArgs*)args)[blockIdx.y]; fql_iqld_loss_critic_body(P, sh); }

struct IqldWeightArgs {
    const float *qa, *qb;      // [B, 16] column 0: the pair (target or online, stored parameters) at (obs, act)
    const float* v;            // [B, 16] column 0: value(obs), stored parameters
    float* w;                  // [B]: loss_weight
    float* rows;               // [3][B]: per-row infos (IQLD_ROWS_*): `o` and `loss_weights` are written here
    float* info;
    int B, mode, topk;         // topk = int(0.1 B), evaluated on the host in double as Python does
    float temp;                // awr_temperature (binary_awr_loss) or softmax_beta (binary_softmax_loss)
};
// agents/iql_diffusion.py:130-168,192-213: adv = min(q1, q2) - v; e = where(adv > 0, clip(exp(adv temp), 0, 1e8), 0);
//   binary: w = adv > 0;  binary_awr_loss: w = min(e, 100);  binary_softmax_loss: w = e / (sum_b e + 1e-8)
// and actor_q, actor_positive_ratio, effective_batch_size = (sum w)^2 / (sum w^2 + 1e-8), max w and the mass of the int(0.1 B) largest
// weights over (sum w + 1e-8).  The largest are selected by rank: rank(b) = #{j : w_j > w_b or (w_j == w_b and j < b)}, so exactly topk
// rows are taken whatever the ties (equal weights contribute equal amounts: the sum is the sorted array's).  topk == 0 takes every row,
// as sorted[-0:] does.  o is all ones in this family: o_mean, o_std, o_min, o_max = 1, 0, 1, 1.
// ws: [2048] in LDS, the weights of a batch of <= 2048 rows: the rank loop below reads each of them B times
__device__ __forceinline__ void fql_iqld_weight_body(const IqldWeightArgs& P, float* sh, float* ws) {
    const int B = P.B;
    float sq = 0.f, sp = 0.f, se = 0.f;
    for (int b = threadIdx.x; b < B; b += FQL_THREADS) {
        const float q = fminf(P.qa[(size_t)b * 16], P.qb[(size_t)b * 16]);
        const float adv = q - P.v[(size_t)b * 16];
        const bool pos = adv > 0.0f;
        float e = 0.f;
        if (pos) e = P.mode == IQLD_BINARY ? 1.0f : fminf(fmaxf(expf(adv * P.temp), 0.0f), 1e8f);
        if (P.mode == IQLD_BINARY_AWR) e = fminf(e, 100.0f);
        P.w[b] = e;
        sq += q;
        sp += pos ? 1.0f : 0.0f;
        se += e;
    }
    const float tq = block_sum(sq, sh), tp = block_sum(sp, sh), te = block_sum(se, sh);
    if (P.mode == IQLD_BINARY_SOFTMAX) {
        const float den = te + 1e-8f;
        for (int b = threadIdx.x; b < B; b += FQL_THREADS) P.w[b] = P.w[b] / den;   // (each thread rewrites its own rows)
    }
    __syncthreads();   // every w[b] is visible to the workgroup
    const bool staged = B <= 2048;
    if (staged) {
        for (int b = threadIdx.x; b < B; b += FQL_THREADS) ws[b] = P.w[b];
        __syncthreads();
    }
    const float* wr = staged ? ws : P.w;   // (larger batches: from global memory, L1 / L2 resident)
    float sw = 0.f, sw2 = 0.f, mx = -INFINITY, st = 0.f;
    for (int b = threadIdx.x; b < B; b += FQL_THREADS) {
        const float wb = wr[b];
        sw += wb;
        sw2 += wb * wb;
        mx = fmaxf(mx, wb);
        P.rows[(size_t)IQLD_ROWS_O * B + b] = 1.0f;
        P.rows[(size_t)IQLD_ROWS_WEIGHTS * B + b] = wb;
        bool take = P.topk == 0;
        if (!take) {
            int rank = 0;
            for (int j = 0; j < B; ++j) {
                const float wj = wr[j];
                rank += (wj > wb || (wj == wb && j < b)) ? 1 : 0;
            }
            take = rank < P.topk;
        }
        if (take) st += wb;
    }
    const float tw = block_sum(sw, sh), tw2 = block_sum(sw2, sh), tt = block_sum(st, sh);
    const float tmx = block_max(mx, sh);
    if (threadIdx.x == 0) {
        float* in = P.info + IQLD_I_ACTOR;
        in[0] = tq / (float)B;              // actor_q
        in[2] = tp / (float)B;              // actor_positive_ratio
        in[5] = 1.0f; in[6] = 0.0f; in[7] = 1.0f; in[8] = 1.0f;   // o_mean, o_std, o_min, o_max
        in[9] = tw * tw / (tw2 + 1e-8f);    // effective_batch_size
        in[10] = tt / (tw + 1e-8f);         // loss_weights_top_10_mass
        in[11] = tmx;                       // loss_weights_max
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_weight_kernel(IqldWeightArgs P) { __shared__ float sh[4]; __shared__ float ws[2048]; fql_iqld_weight_body(P, sh, ws); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_weight_multi_kernel(const IqldWeightArgs* __restrict__ args) { __shared__ float sh[4]; __shared__ float ws[2048]; const IqldWeightArgs P = ((const FQL_CONST_AS IqldWeightArgs*)args)[blockIdx.y]; fql_iqld_weight_body(P, sh, ws); }

struct IqldActorLossArgs {
    const float* pred;         // [2B, ap]: rows [0, B) positive, [B, 2B) unconditional
    const float* vel;          // [B, ap]
    const float* w;            // [B]: loss_weight (a constant under the gradient: stored parameters only)
    float* dpred;              // [2B, ap] or null
    float* rows;               // [3][B]: `actor_losses` is written here
    float* info;
    int B, ad, ap;
};
// agents/iql_diffusion.py:180-189: lp_b = mean_a((vel - pred_pos)^2) w_b, lu_b = mean_a((vel - pred_unc)^2), loss = mean_b(lp + 0.1 lu).
// dL/dpred_pos = -2 w_b (vel - pred) / (B act), dL/dpred_unc = -0.2 (vel - pred) / (B act).  One thread per row.
__device__ __forceinline__ void fql_iqld_loss_actor_body(const IqldActorLossArgs& P, float* sh) {
    const int B = P.B;
    const float gs = 2.0f / ((float)B * (float)P.ad);
    float sp = 0.f, su = 0.f, sl = 0.f;
    for (int b = threadIdx.x; b < B; b += FQL_THREADS) {
        const float wb = P.w[b];
        const float* v = P.vel + (size_t)b * P.ap;
        const size_t op = (size_t)b * P.ap, ou = (size_t)(B + b) * P.ap;
        float ep = 0.f, eu = 0.f;
        for (int a = 0; a < P.ad; ++a) {
            const float dp = v[a] - P.pred[op + a], du = v[a] - P.pred[ou + a];
            ep += dp * dp;
            eu += du * du;
            if (P.dpred) {
                P.dpred[op + a] = -gs * wb * dp;
                P.dpred[ou + a] = -0.1f * gs * du;
            }
        }
        const float lp = ep / (float)P.ad * wb, lu = eu / (float)P.ad;
        const float l = lp + lu * 0.1f;
        P.rows[(size_t)IQLD_ROWS_LOSSES * B + b] = l;
        sp += lp; su += lu; sl += l;
    }
    const float tp = block_sum(sp, sh), tu = block_sum(su, sh), tl = block_sum(sl, sh);
    if (threadIdx.x == 0) {
        float* in = P.info + IQLD_I_ACTOR;
        in[1] = tl / (float)B;   // actor_loss
        in[3] = tp / (float)B;   // actor_loss_positive
        in[4] = tu / (float)B;   // actor_loss_uncond
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_loss_actor_kernel(IqldActorLossArgs P) { __shared__ float sh[4]; fql_iqld_loss_actor_body(P, sh); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_loss_actor_multi_kernel(const IqldActorLossArgs* __restrict__ args) { __shared__ float sh[4]; const IqldActorLossArgs P = ((const FQL_CONST_AS IqldActorLossArgs*)args)[blockIdx.y]; fql_iqld_loss_actor_body(P, sh); }

struct IqldEmbedGradArgs {
    const float* dZ0;          // [2B, H]: gradient at layer 0's pre-activation
    const float* W0e;          // row od + act + 16 of W0 [in_p, H]: the 32 embedding rows
    float* g;                  // [2, 32]: the gradient slot of Embed_0/embedding
    int B, H;
};
// The 32 embedding columns of a half are one constant row, so dEmbed[r] = (column sum over that half of dZ0) W0[embed rows]^T.
// Workgroup 0 takes rows [0, B) (Embed[1]), workgroup 1 rows [B, 2B) (Embed[0]); the column sums run over b in rising order per thread,
// the products over h in rising order.  H <= 1024.  cs: [1024] in LDS.  (The multi-instance grid is (2, members): blockIdx.x stays the half.)
__device__ __forceinline__ void fql_iqld_embed_grad_body(const IqldEmbedGradArgs& P, float* cs) {
    const int half = blockIdx.x;
    const float* dz = P.dZ0 + (size_t)half * P.B * P.H;
    for (int h = threadIdx.x; h < P.H; h += FQL_THREADS) {
        float s = 0.f;
        for (int b = 0; b < P.B; ++b) s += dz[(size_t)b * P.H + h];
        cs[h] = s;
    }
    __syncthreads();
    if (threadIdx.x < IQLD_EMBED) {
        const float* w = P.W0e + (size_t)threadIdx.x * P.H;
        float s = 0.f;
        for (int h = 0; h < P.H; ++h) s = fmaf(cs[h], w[h], s);
        P.g[(half == 0 ? IQLD_EMBED : 0) + threadIdx.x] = s;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_embed_grad_kernel(IqldEmbedGradArgs P) { __shared__ float cs[1024]; fql_iqld_embed_grad_body(P, cs); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_embed_grad_multi_kernel(const IqldEmbedGradArgs* __restrict__ args) { __shared__ float cs[1024]; const IqldEmbedGradArgs P = ((const FQL_CONST_AS IqldEmbedGradArgs*)args)[blockIdx.y]; fql_iqld_embed_grad_body(P, cs); }

struct IqldFinalizeArgs {
    DevState* st;              // the handle's state: the RNG step, and the counters of the critic and value TrainStates
    DevState* st_a;            // the actor TrainState's counters (adam_count, train_step, b1pow, b2pow)
    const float* partials;     // [n_chunks][4]
    const int* leaf_range;     // [nleaves + 1]
    float* info;               // update or probe half of the info buffer
    int leaf_lo, leaf_hi;      // trainable leaves whose gradient statistics are reported: the actor's, else the value net's; lo == hi: none
    int has_value;             // the critic and value losses ran: the value's four infos move from DevState::info (else slots 0-5 are zeroed)
    int has_actor;             // the actor loss ran (else slots 6-17 are zeroed)
    int step_critic, step_actor, advance;
};
// grad/max, grad/min, grad/norm over ONE TrainState's leaves (the reference merges {**critic_info, **value_info, **actor_info}: the
// actor's statistics when it stepped, otherwise the value net's), from the per-chunk partials of that TrainState's Adam launch; the value
// infos in the reference's order (value_loss, v, v_min, v_max); the per-TrainState counters and the RNG step.
// leafn: [256] in LDS.
__device__ __forceinline__ void fql_iqld_finalize_body(const IqldFinalizeArgs& A, float* sh, float* leafn) {
    const int nl = A.leaf_hi - A.leaf_lo;
    float mx = -INFINITY, mn = INFINITY;
    if (nl > 0) {
        const int c0 = A.leaf_range[A.leaf_lo], c1 = A.leaf_range[A.leaf_hi];
        for (int c = c0 + (int)threadIdx.x; c < c1; c += FQL_THREADS) {
            mx = fmaxf(mx, A.partials[4 * c + 1]);
            mn = fminf(mn, A.partials[4 * c + 2]);
        }
        for (int l = threadIdx.x; l < nl; l += FQL_THREADS) {
            float s = 0.f;
            for (int c = A.leaf_range[A.leaf_lo + l]; c < A.leaf_range[A.leaf_lo + l + 1]; ++c) s += A.partials[4 * c];
            leafn[l] = sqrtf(s);
        }
    }
    const float tmx = block_max(mx, sh), tmn = -block_max(-mn, sh);
    __syncthreads();
    if (threadIdx.x != 0) return;
    float* out = A.info;
    if (A.has_value) {
        const float* in = A.st->info + IFQL_I_VALUE;   // value_loss, v_mean, v_max, v_min
        out[IQLD_I_VALUE] = in[0]; out[IQLD_I_VALUE + 1] = in[1]; out[IQLD_I_VALUE + 2] = in[3]; out[IQLD_I_VALUE + 3] = in[2];
    } else {
        for (int i = 0; i < IQLD_I_ACTOR; ++i) out[i] = 0.f;
    }
    if (!A.has_actor)
        for (int i = IQLD_I_ACTOR; i < IQLD_I_GRAD; ++i) out[i] = 0.f;
    float nrm = 0.f;
    for (int i = 0; i < nl; ++i) nrm += leafn[i];
    out[IQLD_I_GRAD] = nl > 0 ? tmx : 0.f;
    out[IQLD_I_GRAD + 1] = nl > 0 ? tmn : 0.f;
    out[IQLD_I_GRAD + 2] = nrm;
    if (A.advance) A.st->rng_step += 1;
    if (A.step_critic) {
        A.st->adam_count += 1; A.st->train_step += 1;
        A.st->b1pow *= 0.9; A.st->b2pow *= 0.999;
    }
    if (A.step_actor) {
        A.st_a->adam_count += 1; A.st_a->train_step += 1;
        A.st_a->b1pow *= 0.9; A.st_a->b2pow *= 0.999;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_finalize_kernel(IqldFinalizeArgs A) { __shared__ float sh[4]; __shared__ float leafn[256]; fql_iqld_finalize_body(A, sh, leafn); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_finalize_multi_kernel(const IqldFinalizeArgs* __restrict__ args) { __shared__ float sh[4]; __shared__ float leafn[256]; const IqldFinalizeArgs A = ((const FQL_CONST_AS IqldFinalizeArgs*)args)[blockIdx.y]; fql_iqld_finalize_body(A, sh, leafn); }

// ---- sample_actions (agents/iql_diffusion.py:249-270) ----------------------------------------------------------------------------
// BC's hoisted form with two halves: z0 = C0 + x W0[act rows] + c[i][half], C0 = obs W0[obs rows] + b0 shared by both halves, and
// c[i][half] = emb[i] W0[emb rows] + Embed[half == 0 ? 1 : 0] W0[embed rows].  Rows [0, n_pad) are the positive half, [n_pad, 2 n_pad)
// the unconditional one; both read the same x.
struct IqldStepBiasArgs {
    const float *emb, *embed;  // [(S + 1), 16]; [2, 32]
    const float* W0e;          // row od + act of W0 [in_p, H]: 16 timestep rows, then 32 embedding rows
    float* Cb;                 // [S, 2, H]
    int S, H;
};
__device__ __forceinline__ void fql_iqld_stepbias_body(const IqldStepBiasArgs& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.S * 2 * P.H) return;
    const int h = e % P.H, half = (e / P.H) & 1, i = e / (2 * P.H);
    const float* row = P.embed + (half == 0 ? IQLD_EMBED : 0);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < BC_EMB; ++j) s = fmaf(P.emb[i * BC_EMB + j], P.W0e[(size_t)j * P.H + h], s);
    for (int j = 0; j < IQLD_EMBED; ++j) s = fmaf(row[j], P.W0e[(size_t)(BC_EMB + j) * P.H + h], s);
    P.Cb[e] = s;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_stepbias_kernel(IqldStepBiasArgs P) { fql_iqld_stepbias_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_stepbias_multi_kernel(const IqldStepBiasArgs* __restrict__ args) { const IqldStepBiasArgs P = ((const FQL_CONST_AS IqldStepBiasArgs*)args)[blockIdx.y]; fql_iqld_stepbias_body(P); }

struct IqldLayer0Args {
    const float *C0, *A, *W0a, *cb;   // C0 [n_pad, H]; A [n_pad, ap]; W0a = row od of W0 (ad rows); cb = rows (i, 0) and (i, 1) of the step-bias table [2, H]
    float* G0;                        // [2 n_pad, H]
    int n_pad, H, ad, ap;
};
// layer 0 of one Euler step for both halves: one thread per (row, column), the act terms in fixed order (as fql_bc_layer0_kernel)
__device__ __forceinline__ void fql_iqld_layer0_body(const IqldLayer0Args& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= 2 * P.n_pad * P.H) return;
    const int r = e / P.H, h = e - r * P.H;
    const int half = r >= P.n_pad ? 1 : 0, src = r - half * P.n_pad;
    float s = P.C0[(size_t)src * P.H + h] + P.cb[half * P.H + h];
    const float* x = P.A + (size_t)src * P.ap;
    for (int a = 0; a < P.ad; ++a) s = fmaf(x[a], P.W0a[(size_t)a * P.H + h], s);
    P.G0[e] = gelu_f(s);
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_layer0_kernel(IqldLayer0Args P) { fql_iqld_layer0_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_layer0_multi_kernel(const IqldLayer0Args* __restrict__ args) { const IqldLayer0Args P = ((const FQL_CONST_AS IqldLayer0Args*)args)[blockIdx.y]; fql_iqld_layer0_body(P); }

struct IqldCfgStepArgs {
    const float* V;            // [2 n_pad, ap]: the head's output, positive half then unconditional half
    float* A;                  // [n_pad, ap]: x, advanced in place
    float* tgt;                // [n_pad, ap]: clip(x) on the last step, else null
    int n_pad, ad, ap;
    float cfg, dt;
};
// v = v_unc + cfg (v_pos - v_unc); x += v dt; the clip after the last step (agents/iql_diffusion.py:263-269)
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_cfg_step_kernel(IqldCfgStepArgs P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.n_pad * P.ad) return;
    const int r = e / P.ad, a = e - r * P.ad;
    const size_t o = (size_t)r * P.ap + a;
    const float vp = P.V[o], vu = P.V[(size_t)P.n_pad * P.ap + o];
    const float v = vu + P.cfg * (vp - vu);
    const float x = P.A[o] + v * P.dt;
    P.A[o] = x;
    if (P.tgt) P.tgt[o] = clip1(x);
}

// ---- guidance sweeps (sample_actions_cfgs): one weight per row ---------------------------------------------------------------------
// The CFG combine and Euler add as fql_iqld_cfg_step_kernel's code object rounds them (v_sub, v_fmac, v_fmac): t = vp - vu; v = c t + vu;
// x + v dt.  Spelled with fmaf so that the rounding is the source's, not an optimiser's choice per kernel body: a subtraction feeding
// an fma cannot contract, and nothing else here is a bare multiply-add.
__device__ __forceinline__ float iqld_cfg_euler(float x, float vp, float vu, float c, float dt) {
    const float t = vp - vu;
    const float v = fmaf(c, t, vu);
    return fmaf(v, dt, x);
}

struct IqldCfgRowsStepArgs {
    const float* V;            // [2 n_pad, ap]: the head's output, positive half then unconditional half
    const float* X;            // [n_pad, ap]: x before the step (the ping-pong buffer that holds it)
    const float* cfg;          // [n_pad]: the weight of each source row (0 for rows >= n)
    float* tgt;                // [n_pad, ap]: clip(x + v dt)
    int n_pad, ad, ap;
    float dt;
};
// the last Euler step of a sweep program: fql_iqld_cfg_step_kernel with the row's own weight; x itself is not written back
__device__ __forceinline__ void fql_iqld_cfg_rows_step_body(const IqldCfgRowsStepArgs& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.n_pad * P.ad) return;
    const int r = e / P.ad, a = e - r * P.ad;
    const size_t o = (size_t)r * P.ap + a;
    P.tgt[o] = clip1(iqld_cfg_euler(P.X[o], P.V[o], P.V[(size_t)P.n_pad * P.ap + o], P.cfg[r], P.dt));
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_cfg_rows_step_kernel(IqldCfgRowsStepArgs P) { fql_iqld_cfg_rows_step_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_cfg_rows_step_multi_kernel(const IqldCfgRowsStepArgs* __restrict__ args) { const IqldCfgRowsStepArgs P = ((const FQL_CONST_AS IqldCfgRowsStepArgs*)args)[blockIdx.y]; fql_iqld_cfg_rows_step_body(P); }

struct IqldCfgLayer0Args {
    const float *C0, *V, *Xin, *cfg, *W0a, *cb;   // C0 [n_pad, H]; V [2 n_pad, ap]: the previous step's head output; Xin [n_pad, ap]; cfg [n_pad];
                                                  // W0a = row od of W0 (ad rows); cb = rows (i, 0) and (i, 1) of the step-bias table [2, H]
    float *Xout, *G0;                             // Xout [n_pad, ap]: x after the previous step's Euler add (the other ping-pong buffer); G0 [2 n_pad, H]
    int n_pad, H, ad, ap;
    float dt;
};
// Euler step i >= 1 of a sweep program in one launch: the CFG combine and Euler add of step i - 1 (fql_iqld_cfg_step_kernel's
// arithmetic, the row's own weight), then layer 0 of step i on the new x (fql_iqld_layer0_kernel's: C0 + cb, the act terms in rising
// order, GELU).  One thread per (row, column) as there; every thread forms the ad values x_new[src][.] it multiplies (a wave reads one
// row: the loads are broadcasts).  Xin is read and Xout written, so no thread reads what another writes; the positive half's threads
// h, h + H, .. < ap store x_new (0 in the padding columns) for the next launch.
__device__ __forceinline__ void fql_iqld_cfg_layer0_body(const IqldCfgLayer0Args& P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= 2 * P.n_pad * P.H) return;
    const int r = e / P.H, h = e - r * P.H;
    const int half = r >= P.n_pad ? 1 : 0, src = r - half * P.n_pad;
    float s = P.C0[(size_t)src * P.H + h] + P.cb[half * P.H + h];
    const float* x = P.Xin + (size_t)src * P.ap;
    const float* vp = P.V + (size_t)src * P.ap;
    const float* vu = P.V + (size_t)(P.n_pad + src) * P.ap;
    const float c = P.cfg[src];
    for (int a = 0; a < P.ad; ++a) s = fmaf(iqld_cfg_euler(x[a], vp[a], vu[a], c, P.dt), P.W0a[(size_t)a * P.H + h], s);
    P.G0[e] = gelu_f(s);
    if (half == 0)
        for (int a = h; a < P.ap; a += P.H)
            P.Xout[(size_t)src * P.ap + a] = a < P.ad ? iqld_cfg_euler(x[a], vp[a], vu[a], c, P.dt) : 0.f;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_cfg_layer0_kernel(IqldCfgLayer0Args P) { fql_iqld_cfg_layer0_body(P); }
__global__ __launch_bounds__(FQL_THREADS) void fql_iqld_cfg_layer0_multi_kernel(const IqldCfgLayer0Args* __restrict__ args) { const IqldCfgLayer0Args P = ((const FQL_CONST_AS IqldCfgLayer0Args*)args)[blockIdx.y]; fql_iqld_cfg_layer0_body(P); }

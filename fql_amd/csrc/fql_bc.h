// fql_bc.h -- the kernels of the BC agent (agents/bc.py) that FQL's kernels do not cover: batch assembly with the timestep embedding,
// the 4-info finalize, and the sampler's input rows, step-bias table and layer 0.  The GEMM bodies (LayerNorm on the A tile), weight gradients, LayerNorm backward,
// the flow-matching loss (fql_loss_bc_body: its 2 / (B act) scaling is BC's), Adam and the grad statistics are FQL's; the sampler's
// Euler add and final clip ride in the head GEMM's epilogue (GF_EULER | GF_EULER_BARE, fql_kernels.h).
#pragma once
#include "fql_kernels.h"

// Timestep embedding (agents/bc.py:15-24): [cos(arg_i) | sin(arg_i)], i = 0..7.  t only takes the S + 1 grid values k / S, so the
// [(S + 1), 16] table is built on the host at create (fp64 cos / sin of the fp32 argument) and indexed by k.
enum : int { BC_EMB = 16 };
// Info slots while a BC update runs: the loss body writes slot 5 and FQL's finalize slots 10-12; fql_bc_finalize_kernel moves them
// into the reference's order (agents/bc.py:80-84 + utils/flax_utils.py:132-159): bc_loss, grad/max, grad/min, grad/norm
enum : int { BC_I_LOSS = 5 };

struct BcPrepArgs {
    const SrcDesc* src;
    DevState* st;
    uint64_t key;
    const float* emb;          // [(S + 1), 16]
    int B, od, ad;
    int inp, ap, S;            // padded input width of the policy (od + ad + 16), padded action width, denoise_steps
    float *X, *vel;            // [B, inp], [B, ap]
};
// utils/datasets.py:64-100 (index draw + gather), agents/bc.py:56-66 (x_0, k, x_t, vel): one wave per transition writes
// X = [obs | x_t | emb[k] | 0] and vel = act - x_0.  x_0 is Philox tensor 2 (as FQL's BC-flow noise), k = floor(u32 (S + 1) / 2^32) of
// tensor 3; explicit tensors replace them (S.t holds t = k / S, read as round(t S)).
__global__ __launch_bounds__(FQL_THREADS) void fql_bc_prep_kernel(BcPrepArgs P) {
    const SrcDesc& S = *P.src;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= P.B) return;
    const uint64_t step = P.st->rng_step;
    const uint64_t key = P.key ^ (P.st->rng_stream * 0x9E3779B97F4A7C15ull);
    int64_t src = b;
    if (S.idx) src = S.idx[b];
    else if (S.use_rng_idx) src = S.lo + (int64_t)(((uint64_t)rng_u32(key, step, 7u, (uint32_t)b) * (uint64_t)S.span) >> 32);
    const int od = P.od, ad = P.ad;
    const float* obs = S.obs + (size_t)src * od;
    const float* act = S.act + (size_t)src * ad;
    int k = S.t ? (int)rintf(S.t[b] * (float)P.S) : (int)(((uint64_t)rng_u32(key, step, 3u, (uint32_t)b) * (uint64_t)(P.S + 1)) >> 32);
    k = k < 0 ? 0 : (k > P.S ? P.S : k);
    const float tt = (float)k / (float)P.S;
    const float* em = P.emb + (size_t)k * BC_EMB;
    for (int j = lane; j < P.inp; j += 64) {
        float v = 0.f;
        if (j < od) v = obs[j];
        else if (j < od + ad) {
            const int a = j - od;
            const float av = act[a];
            const float xx = S.x0 ? S.x0[(size_t)b * ad + a] : rng_normal(key, step, 2u, (uint32_t)b, (uint32_t)a);
            v = (1.0f - tt) * xx + tt * av;                      // bc.py:64
            P.vel[(size_t)b * P.ap + a] = av - xx;               // bc.py:65
        } else if (j < od + ad + BC_EMB) v = em[j - od - ad];
        P.X[(size_t)b * P.inp + j] = v;
    }
}

// FQL's finalize (grad statistics into slots 10-12 and the step counters), then the reference's BC order in slots 0-3
__global__ __launch_bounds__(FQL_THREADS) void fql_bc_finalize_kernel(FinalizeArgs A) {
    fql_finalize_body(A);
    if (threadIdx.x == 0) {
        float* in = A.st->info;
        const float loss = in[BC_I_LOSS], gmax = in[10], gmin = in[11], gn = in[12];
        in[0] = loss; in[1] = gmax; in[2] = gmin; in[3] = gn;
    }
}

// ---- sample_actions (agents/bc.py:86-101) -----------------------------------------------------------------------------------------
// Layer 0 of step i is z0 = [obs | x | emb[i]] W0 + b0 = C0 + x W0[act rows] + c_i with the loop-invariant C0 = obs W0[obs rows] + b0
// (one GEMM per call) and the step bias c_i = emb[i] W0[emb rows] (every row of a step shares t): per step a rank-act update and a row add.
struct BcAssembleArgs {
    const float *obs, *noise;  // obs [n, od]; noise [n, ad] or null (Philox keyed by (key, seed))
    float* X;                  // [n_pad, inp]: row r = [obs_r | 0]; rows >= n are zero
    float* A;                  // [n_pad, ap]: x_r (the flow's state); padding columns and rows >= n are zero
    uint64_t key, seed;
    int n, n_pad, od, ad, inp, ap;
    int row0;                  // index of this chunk's first row in the call (keys the Philox draw: chunking does not change the noise)
};
__device__ __forceinline__ void fql_bc_assemble_body(const BcAssembleArgs& P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= P.n_pad) return;
    for (int j = lane; j < P.inp; j += 64) P.X[(size_t)r * P.inp + j] = (r < P.n && j < P.od) ? P.obs[(size_t)r * P.od + j] : 0.f;
    for (int a = lane; a < P.ap; a += 64) {
        float v = 0.f;
        if (r < P.n && a < P.ad) v = P.noise ? P.noise[(size_t)r * P.ad + a] : rng_normal(P.key, P.seed, 12u, (uint32_t)(P.row0 + r), (uint32_t)a);
        P.A[(size_t)r * P.ap + a] = v;
    }
}
__global__ __launch_bounds__(FQL_THREADS) void fql_bc_assemble_kernel(BcAssembleArgs P) { fql_bc_assemble_body(P); }
// Multi-instance entry point (IQL-diffusion agent groups, whose sampler assembles its rows with this kernel): blockIdx.y picks the
// member, its argument struct comes from a device array, read through the constant address space (fql_kernels.h FQL_CONST_AS)
__global__ __launch_bounds__(FQL_THREADS) void fql_bc_assemble_multi_kernel(const BcAssembleArgs* __restrict__ args) { const BcAssembleArgs P = ((const FQL_CONST_AS BcAssembleArgs*)args)[blockIdx.y]; fql_bc_assemble_body(P); }

// the [S, H] step-bias table: Cb[i][h] = sum_j emb[i][j] W0[od + ad + j][h], j in fixed order
struct BcStepBiasArgs {
    const float *emb, *W0e;    // emb [(S + 1), 16]; W0e = row od + ad of W0 [in_p, H] (16 rows)
    float* Cb;                 // [S, H]
    int S, H;
};
__global__ __launch_bounds__(FQL_THREADS) void fql_bc_stepbias_kernel(BcStepBiasArgs P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.S * P.H) return;
    const int i = e / P.H, h = e - i * P.H;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < BC_EMB; ++j) s = fmaf(P.emb[i * BC_EMB + j], P.W0e[(size_t)j * P.H + h], s);
    P.Cb[e] = s;
}

// layer 0 of one Euler step: G0 = GELU(C0 + x W0[act rows] + c_i); one thread per (row, column), the act terms in fixed order
struct BcLayer0Args {
    const float *C0, *A, *W0a, *cb;   // C0 [M, H]; A [M, ap]; W0a = row od of W0 [in_p, H] (ad rows); cb = row i of the step-bias table [H]
    float* G0;                        // [M, H]
    int M, H, ad, ap;
};
__global__ __launch_bounds__(FQL_THREADS) void fql_bc_layer0_kernel(BcLayer0Args P) {
    const int e = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (e >= P.M * P.H) return;
    const int r = e / P.H, h = e - r * P.H;
    float s = P.C0[e] + P.cb[h];
    const float* x = P.A + (size_t)r * P.ap;
    for (int a = 0; a < P.ad; ++a) s = fmaf(x[a], P.W0a[(size_t)a * P.H + h], s);
    P.G0[e] = gelu_f(s);
}

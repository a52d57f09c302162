// Kernels off the update's hot path, kept in a header of their own that is included LAST: code inserted in front of the GEMM-family
// kernels shifts their placement in the code object, which was measured to move the update rate by ~1 % (same box, A/B of builds).
#pragma once
#include "fql_kernels.h"

// ------------------------------------------------------------------------------------------------
// JAX-compatible noise on the device: the five tensors of one update from the five keys the reference's split
// chain derives (agents/fql.py:24,49-54,62-63,82,125,143-150; fql_amd/jax_prng.py restates the chain and both counter layouts).
// jax.random.normal = sqrt(2) erf_inv(uniform(nextafter(-1, 0), 1)), jax.random.uniform = (bits >> 9 | 0x3f800000) - 1 scaled;
// bits = Threefry-2x32 (20 rounds) in the original layout (counter array cut in two halves) or the partitionable one (counter =
// element index, output = word 0 ^ word 1).  erf_inv: the single-precision Giles polynomial XLA evaluates.
// ------------------------------------------------------------------------------------------------
struct JaxNoiseArgs {
    uint32_t key[5][2];   // eps1, x0, t, z, eps2
    float* out[5];
    int n[5];             // elements of each: B ad, B ad, B, B ad, B ad
    int partitionable;
};
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
    const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
    x0 += ks[0]; x1 += ks[1];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int r0[4] = {13, 15, 26, 6}, r1[4] = {17, 29, 16, 24};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x0 += x1;
            x1 = rotl32(x1, (i & 1) ? r1[j] : r0[j]);
            x1 ^= x0;
        }
        x0 += ks[(i + 1) % 3];
        x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
    }
}
__device__ __forceinline__ float erfinv_giles(float x) {
    float w = -logf(__fmul_rn(1.0f - x, 1.0f + x));
    float p;
    if (w < 5.0f) {
        w = w - 2.5f;
        p = 2.81022636e-08f;
        p = 3.43273939e-07f + p * w;
        p = -3.5233877e-06f + p * w;
        p = -4.39150654e-06f + p * w;
        p = 0.00021858087f + p * w;
        p = -0.00125372503f + p * w;
        p = -0.00417768164f + p * w;
        p = 0.246640727f + p * w;
        p = 1.50140941f + p * w;
    } else {
        w = sqrtf(w) - 3.0f;
        p = -0.000200214257f;
        p = 0.000100950558f + p * w;
        p = 0.00134934322f + p * w;
        p = -0.00367342844f + p * w;
        p = 0.00573950773f + p * w;
        p = -0.0076224613f + p * w;
        p = 0.00943887047f + p * w;
        p = 1.00167406f + p * w;
        p = 2.83297682f + p * w;
    }
    return p * x;
}
__global__ __launch_bounds__(FQL_THREADS) void fql_jax_noise_kernel(const JaxNoiseArgs P) {
    const int which = blockIdx.y;
    int n = 0; float* out = nullptr; uint32_t k0 = 0, k1 = 0;
#pragma unroll
    for (int w = 0; w < 5; ++w) if (w == which) { n = P.n[w]; out = P.out[w]; k0 = P.key[w][0]; k1 = P.key[w][1]; }
    const int i = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t x0, x1, bits;
    if (P.partitionable) {
        x0 = 0u; x1 = (uint32_t)i;
        threefry2x32(k0, k1, x0, x1);
        bits = x0 ^ x1;
    } else {
        const int half = (n + 1) >> 1;
        const int j = i < half ? i : i - half;
        x0 = (uint32_t)j; x1 = (j + half < n) ? (uint32_t)(j + half) : 0u;   // odd sizes: the counter array is padded with one zero
        threefry2x32(k0, k1, x0, x1);
        bits = i < half ? x0 : x1;
    }
    const float fl = __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f;
    if (which == 2) {                      // t ~ uniform(0, 1)
        out[i] = fmaxf(0.0f, fl);
    } else {                               // normal: minval = nextafter(-1, 0), maxval - minval rounds to 2 in float32
        const float lo = __uint_as_float(0xBF7FFFFFu);
        const float u = fmaxf(lo, __fadd_rn(__fmul_rn(fl, 2.0f), lo));
        out[i] = 1.41421354f * erfinv_giles(u);
    }
}

// ------------------------------------------------------------------------------------------------
// Module queries (fql_module_forward: agent.network.select(module)(...), utils/flax_utils.py ModuleDict / TrainState.select).
// ------------------------------------------------------------------------------------------------
// The padded input rows of one chunk: row r = [obs_r | act_r | t_r | 0] (utils/networks.py Value.__call__ concatenates
// [observations, actions], ActorVectorField.__call__ [observations, actions, times]); act and t may be null (the module takes none),
// rows >= n and the pad columns are zero.  One wave per row, as fql_assemble_kernel; no RNG.
struct QueryAssembleArgs {
    const float *obs, *act, *t;   // [n, od], [n, ad] or null, [n] or null
    float* X;                     // [n_pad, inp]
    int n, n_pad, od, ad, inp;
};
__global__ __launch_bounds__(FQL_THREADS) void fql_query_assemble_kernel(const QueryAssembleArgs P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= P.n_pad) return;
    const int a1 = P.od + (P.act ? P.ad : 0);   // first column behind the action block
    for (int j = lane; j < P.inp; j += 64) {
        float v = 0.f;
        if (r < P.n) {
            if (j < P.od) v = P.obs[(size_t)r * P.od + j];
            else if (j < a1) v = P.act[(size_t)r * P.ad + (j - P.od)];
            else if (j == a1 && P.t) v = P.t[r];
        }
        P.X[(size_t)r * P.inp + j] = v;
    }
}
// The scalar heads of one chunk: out[e ld + r] = q_e[r, 0] for the `members` (1: value, 2: the critic pair) padded head outputs
// [n_pad, 16], in one launch.  out points at the chunk's first row of member 0; ld is the member stride (the call's n for a device
// `out`, the chunk's rows for the staging buffer).
struct QueryHeadsArgs {
    const float* q[2];   // [n_pad, 16] column 0; q[1] is null for one member
    float* out;
    int n, members;
    size_t ld;
};
__global__ __launch_bounds__(FQL_THREADS) void fql_query_heads_kernel(const QueryHeadsArgs P) {
    const int i = blockIdx.x * FQL_THREADS + threadIdx.x;
    if (i >= P.n * P.members) return;
    const int e = i >= P.n, r = i - e * P.n;
    P.out[(size_t)e * P.ld + r] = (e ? P.q[1] : P.q[0])[(size_t)r * 16];
}

// ------------------------------------------------------------------------------------------------
// A group's sampling call (fql_group_sample_actions, fql_group_flow_actions): multi-instance entry points of fql_assemble_kernel and
// fql_extract_kernel (fql_kernels.h, bodies shared).  blockIdx.y picks the member, its argument struct comes from a device array, read
// through the constant address space (scalar loads, as from the kernel-argument segment).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FQL_THREADS) void fql_assemble_multi_kernel(const AssembleArgs* __restrict__ args) { const AssembleArgs P = ((const FQL_CONST_AS AssembleArgs*)args)[blockIdx.y]; fql_assemble_body(P); }
// the single-instance kernel's arguments as a struct, one per member
struct ExtractArgs {
    const float* src;
    float* out;
    int n, ad, ap;
};
__global__ void fql_extract_multi_kernel(const ExtractArgs* __restrict__ args) { const ExtractArgs P = ((const FQL_CONST_AS ExtractArgs*)args)[blockIdx.y]; fql_extract_body(P.src, P.out, P.n, P.ad, P.ap); }

// FQL step engine for MI355X (gfx950): host side + C ABI (include/fql_amd.h).
//
// One stateful engine owns every device buffer of the step (params, Adam state, target network,
// activations, dataset).  A training step is written ONCE as a straight-line program of tile tasks
// with explicit read/write sets; a list scheduler levels the program (RAW/WAR/WAW on buffers), all
// tasks of one kernel type in one level become ONE launch driven by a task table in HBM, and the
// level sequence is captured into a hipGraph.  The kernel boundary is the only grid-wide barrier used
// (cheapest on gfx950: ~1.3 us vs >4 us for an in-kernel grid barrier).
//
// Reference behaviour being replaced: agents/fql.py:22-171, utils/networks.py:34-61,153-235,
// utils/flax_utils.py:90-159, utils/datasets.py:64-100,435-495 (zhouzypaul/fql).
//
// This file is the translation unit.  One layer of it lies in a header beside it, a part of this unit and not a unit of its own:
//   fql_engine_groups.h   the agent-group layer and its C entry points (included at the end of this file)
#include "../../include/fql_amd.h"
#include "fql_kernels.h"
#include "fql_conv.h"
#include "fql_chain.h"
#include "fql_aux.h"
#include "fql_ifql.h"
#include "fql_rebrac.h"
#include "fql_sac.h"
#include "fql_bc.h"
#include "fql_iql.h"
#include "fql_iqld.h"
#include "fql_cfgrl.h"
#include <hip/hip_ext.h>
#include "fql_aql.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#define FQL_LANES 4

// The code object holds the template kernels in the order they are instantiated, which would otherwise be the order in which the host code
// below happens to name them.  It is fixed here: with the same ISA in every kernel, another placement alone moved the update rate by 0.4 %
// (MEASUREMENTS.md, "Every launch bound when built").
template __global__ void fql_gemm16_euler_kernel<true>(const GemmTask*, int, int);
template __global__ void fql_gemm16_euler_kernel<false>(const GemmTask*, int, int);
template __global__ void fql_gemm16_kernel<true>(const GemmTask*, int, int);
template __global__ void fql_gemm16_kernel<false>(const GemmTask*, int, int);
template __global__ void fql_chain_split_kernel<512, 0>(ChainArgs); template __global__ void fql_chain_split_kernel<512, 1>(ChainArgs); template __global__ void fql_chain_split_kernel<512, 2>(ChainArgs);
template __global__ void fql_chain_split_kernel<256, 0>(ChainArgs); template __global__ void fql_chain_split_kernel<256, 1>(ChainArgs); template __global__ void fql_chain_split_kernel<256, 2>(ChainArgs);
template __global__ void fql_chain_kernel<512, 0>(ChainArgs); template __global__ void fql_chain_kernel<512, 1>(ChainArgs); template __global__ void fql_chain_kernel<512, 2>(ChainArgs); template __global__ void fql_chain_kernel<512, 3>(ChainArgs);
template __global__ void fql_chain_kernel<256, 0>(ChainArgs); template __global__ void fql_chain_kernel<256, 1>(ChainArgs); template __global__ void fql_chain_kernel<256, 2>(ChainArgs); template __global__ void fql_chain_kernel<256, 3>(ChainArgs);

namespace {

thread_local std::string g_create_error;

struct HipError {
    std::string msg;
};
#define HIP_CHECK(expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            char buf_[512];                                                                          \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            throw HipError{buf_};                                                                    \
        }                                                                                            \
    } while (0)

struct Invalid {
    std::string msg;
};
[[noreturn]] void invalid(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Invalid{buf};
}

inline int pad16(int x) { return (x + 15) & ~15; }

// ------------------------------------------------------------------------------------------------
// networks in the parameter arena
// ------------------------------------------------------------------------------------------------
struct Layer {
    int in, out, in_p, out_p;
    size_t w, b;      // arena offsets (floats)
    bool ln;          // LayerNorm after this layer's GELU
    size_t g, be;     // LN scale / bias offsets
};
struct Net {
    std::vector<Layer> layers;
    size_t off = 0, size = 0;
    int in() const { return layers.front().in; }
    int in_p() const { return layers.front().in_p; }
    int nl() const { return (int)layers.size(); }
};
// NET_TA: ReBRAC's target actor (empty, zero-sized, in every other agent: their arena is unchanged)
enum { NET_C0 = 0, NET_C1, NET_BC, NET_OS, NET_T0, NET_T1, NET_TA, NUM_NETS };

// IMPALA encoder in the arena (utils/encoders.py:61-100): per stack 1 + 2 num_blocks convolutions, then Dense + GELU.
// A convolution leaf is stored exactly as flax lays it out, [3][3][cin][cout] = [tap][cin][cout], bias [cout].
struct ConvL {
    size_t w, b;
    int cin, cout;
    float *Wf = nullptr, *Wb = nullptr;   // LDS-layout copies refreshed by fql_conv_wprep_kernel at the start of each pass
    bool split = false;                   // precision = 2: the copies are bf16 hi / lo planes (fql_conv3x3_split_kernel)
    bool pool_fused = false;              // a stack's first convolution that runs fused with the stack's max-pool (fp32 forward copy in both precisions)
};
struct EncStack {
    std::vector<ConvL> conv;  // conv[0] at the stack's input resolution, the rest after the 2x max-pool
    int H, W;                 // input resolution of the stack
};
struct EncNet {
    std::vector<EncStack> stacks;
    Layer dense;              // flat -> enc_dim
    int flat = 0;
    size_t off = 0, size = 0;
};
enum { ENC_C = 0, ENC_BC, ENC_OS, ENC_T, NUM_ENC };
inline int pad16c(int c) { return (c + 15) & ~15; }

struct Segment {  // one contiguous padded block of a leaf
    size_t off;
    int rows, cols, rows_p, cols_p;  // logical and padded 2-D shape (vectors: rows = 1)
    int chunk_w = 0;                 // > 0: a column block of a wider layer (SAC's actor heads): Adam chunks of chunk_w floats per padded row
};
struct Leaf {
    std::string name;
    int ndim;
    int64_t shape[4];
    std::vector<Segment> segs;  // 1 (actors) or 2 (ensemble members)
    bool trainable;
    int train_id;  // index among trainable leaves or -1
};

// ------------------------------------------------------------------------------------------------
// program = ordered ops with read/write sets -> levels -> launches
// ------------------------------------------------------------------------------------------------
// OP_WGRAD, OP_LNBWD, OP_POSTOS and the OP_LOSS_{CRITIC,Q,BC} ops ride in OP_GEMM64 (side-lane) launches, never in launches of their own.
// OP_PEC and OP_XCHAIN are reserved (retired persistent Euler chains): the values index profile labels (bench.py OP_NAMES) and order launches.
// A type is a label (fql_debug_plan, FQL_TRACE, FQL_DUMP, the profile pass, bench.py OP_NAMES) and the sort key inside a (level, lane) of
// schedule(); it does not say how a launch is issued.  Every launch is a Bound (below): the ops that are launches of their own (OP_PREP,
// OP_EULER_FIN, OP_LOSS_ACTOR, OP_POOL, OP_POOL_BWD, OP_ENC_DZ, OP_CHAIN, OP_WFRAG, OP_HEAD_DGRAD, OP_ADAM, OP_FINALIZE, an unmerged
// OP_CONV_WPREP and every agent type, OP_IFQL_PREP and later) are bound where they are emitted (fql_engine::emit()); the types whose ops
// schedule() merges per level (OP_GEMM, OP_GEMM64 with its riders, the convolution families, OP_DGRAD0, merged OP_CONV_WPREP) carry a payload
// in Op and are bound where schedule() forms the launch.  A new kernel adds an enum label and an emit site: no member of Op, nothing in issue().
enum OpType { OP_GEMM, OP_GEMM64, OP_WGRAD, OP_LNBWD, OP_PREP, OP_POSTOS, OP_EULER_FIN, OP_PEC, OP_LOSS_CRITIC, OP_LOSS_Q, OP_LOSS_BC,
              OP_LOSS_ACTOR, OP_CONV_WPREP, OP_CONV, OP_CONV_U8, OP_POOL, OP_POOL_BWD, OP_CONV_WGRAD, OP_CONV_WRED, OP_ENC_DZ, OP_CHAIN, OP_WFRAG, OP_XCHAIN, OP_HEAD_DGRAD, OP_DGRAD0, OP_ADAM,
              OP_FINALIZE,
              // IFQL (agents/ifql.py) only: after every FQL type, so FQL programs keep their launch order
              OP_IFQL_PREP, OP_IFQL_LOSS_V, OP_IFQL_LOSS_C, OP_IFQL_FIN,
              // ReBRAC (agents/rebrac.py) only: after IFQL's
              OP_REBRAC_PREP, OP_REBRAC_ACT, OP_REBRAC_LOSS_C, OP_REBRAC_LOSS_A, OP_REBRAC_AGRAD, OP_REBRAC_FIN,
              // SAC (agents/sac.py) only: after ReBRAC's
              OP_SAC_PREP, OP_SAC_ACT, OP_SAC_LOSS_C, OP_SAC_LOSS_A, OP_SAC_AGRAD, OP_SAC_FIN,
              // BC (agents/bc.py) only: after SAC's
              OP_BC_PREP, OP_BC_FIN, OP_BC_STEPBIAS, OP_BC_LAYER0,
              // IQL (agents/iql.py) only: after BC's
              OP_IQL_PREP, OP_IQL_HEAD, OP_IQL_LOSS_AWR, OP_IQL_LOSS_DDPGBC, OP_IQL_AGRAD, OP_IQL_FIN,
              // IQL-diffusion (agents/iql_diffusion.py) only: after IQL's
              OP_IQLD_PREP, OP_IQLD_LOSS_C, OP_IQLD_WEIGHT, OP_IQLD_LOSS_A, OP_IQLD_EGRAD, OP_IQLD_FIN, OP_IQLD_STEPBIAS, OP_IQLD_LAYER0,
              OP_IQLD_CFG,
              // CFGRL (agents/cfgrl.py) only: after IQL-diffusion's
              OP_CFGRL_PREP, OP_CFGRL_EGRAD, OP_CFGRL_FIN, OP_CFGRL_LAYER0,
              // the sweep programs of both CFG samplers (one guidance weight per row): after CFGRL's
              OP_CFG_ROWS_LAYER0, OP_CFG_ROWS_STEP, OP_NUM_TYPES };

// One dispatch, complete: the kernel, its grid, block and dynamic LDS bytes, and the arguments packed as the kernarg segment lays them out.
// Every launch of every program is one of these, bound where the launch is formed - at the emit site of a single-op launch (fql_engine::emit()),
// in schedule() for the launches that merge the ops of a level - and issue() launches it as it stands.
constexpr int FQL_BOUND_ARGS = 11;      // (the table form of the side kernels)
constexpr int FQL_BOUND_BYTES = 4096;   // a launch's arguments never exceed the kernarg segment (FQL_KA_LIMIT and the hidden block)
struct Bound {
    const void* fn = nullptr;   // the kernel's host address; null: the op carries no bound launch
    unsigned grid[3] = {1, 1, 1}, block[3] = {FQL_THREADS, 1, 1};
    unsigned lds = 0;           // dynamic LDS bytes
    int nargs = 0;
    int at[FQL_BOUND_ARGS] = {};   // byte offset of each argument
    int tl_at = -1;             // byte offset of the int that receives the timeline id at issue time, -1: none
    std::vector<uint8_t> args;
    unsigned workgroups() const { return grid[0] * grid[1] * grid[2]; }
};
// grid, block and LDS bytes of a bound launch; a plain workgroup count means FQL_THREADS threads and no LDS
struct Geo {
    dim3 grid, block;
    size_t lds;
    Geo(int g) : grid((unsigned)g), block(FQL_THREADS), lds(0) {}
    Geo(dim3 g, dim3 b, size_t l) : grid(g), block(b), lds(l) {}
};
template <typename... T>
constexpr size_t packed_bytes() {   // kernarg layout: every argument at its natural alignment
    size_t off = 0;
    ((off = ((off + alignof(T) - 1) & ~(alignof(T) - 1)) + sizeof(T)), ...);
    return off;
}
// kernel and arguments meet here, at compile time: each argument is converted to the kernel's parameter type and packed as the kernarg
// segment lays it out
template <typename... Pm, typename... A>
Bound bind(void (*k)(Pm...), Geo g, A&&... a) {
    static_assert(sizeof...(Pm) == sizeof...(A) && sizeof...(Pm) <= FQL_BOUND_ARGS, "a bound launch takes exactly the kernel's arguments");
    static_assert(packed_bytes<Pm...>() <= FQL_BOUND_BYTES, "arguments larger than a kernarg segment");
    Bound b;
    b.fn = (const void*)k;
    b.grid[0] = g.grid.x; b.grid[1] = g.grid.y; b.grid[2] = g.grid.z;
    b.block[0] = g.block.x; b.block[1] = g.block.y; b.block[2] = g.block.z;
    b.lds = (unsigned)g.lds;
    b.args.resize(packed_bytes<Pm...>());
    size_t off = 0;
    auto put = [&](auto v) {
        using T = decltype(v);
        off = (off + alignof(T) - 1) & ~(alignof(T) - 1);
        b.at[b.nargs++] = (int)off;
        std::memcpy(b.args.data() + off, &v, sizeof(T));
        off += sizeof(T);
    };
    (put(static_cast<Pm>(a)), ...);
    return b;
}
// the same launch with the timeline id written, at issue time, `off` bytes into its first argument / into its last argument (an int)
inline Bound tl_in(Bound k, size_t off) { k.tl_at = k.at[0] + (int)off; return k; }
inline Bound tl_last(Bound k) { k.tl_at = k.at[k.nargs - 1]; return k; }
// The one launch body: bound launch k with the argument bytes `args` (k.args, or a copy with the issue-time words written) on stream s.
// pa / pb set: the dispatch carries the two events (fql_profile_update).
inline void launch_bound(const Bound& k, const void* args, hipStream_t s, hipEvent_t pa = nullptr, hipEvent_t pb = nullptr) {
    void* argv[FQL_BOUND_ARGS];
    for (int i = 0; i < k.nargs; ++i) argv[i] = (unsigned char*)args + k.at[i];
    const dim3 g(k.grid[0], k.grid[1], k.grid[2]), b(k.block[0], k.block[1], k.block[2]);
    if (pa) (void)hipExtLaunchKernel(k.fn, g, b, argv, k.lds, s, pa, pb, 0);
    else (void)hipLaunchKernel(k.fn, g, b, argv, k.lds, s);
}

// An op is a launch of its own (k is bound, no payload) or a task that schedule() merges with the others of its level, lane and family into
// one launch (a payload below, k unbound).
struct Op {
    OpType type;
    std::vector<const void*> reads, writes;
    GemmTask gemm;
    WgradTask wgrad;
    LnBwdTask ln;
    PostOsArgs postos;
    LossCriticArgs lc;
    LossQArgs lq;
    LossBcArgs lb;
    ConvArgs conv;
    ConvWgradArgs cw;
    ConvWredArgs cwr;
    const ConvWprepTask* wprep_tasks = nullptr;
    int wprep_n = 0;
    int cw_grid = 0;
    Bound k;                 // single-op launches: the launch, bound where the op is emitted
    double macs = 0.0;       // ... and its algorithmic multiply-accumulates where its payload does not say them (chain launches)
    int level = 0;
    int lane = 0;            // 0 = critical lane (Euler chain, one-step backward), 1 = side lane
    int launch = -1;         // index of the launch schedule() put this op into
    std::vector<int> deps;   // indices of earlier ops this op must follow (RAW / WAW / WAR)
};

// What issue() needs of a launch is its Bound; the rest is what the diagnostics report, what orders the lanes, and what an agent group needs
// to fuse the members' table-driven launches.
struct Launch {
    Launch() = default;
    Launch(OpType t, int ln) : type(t), lane(ln) {}
    OpType type;
    int lane = 0;
    int grid = 0, ntasks = 0;    // table-driven launches: workgroups and tasks (0 in a single-op launch; fql_profile_update, FQL_TRACE, FQL_DUMP)
    Bound k;
    double macs = 0.0;           // algorithmic multiply-accumulates of the GEMM-shaped tasks of this launch (roofline accounting)
    void* table = nullptr;       // device task table (GEMM / GEMM64 / convolution families)
    // OP_GEMM64 (side-lane) launches: gemm64 tiles, then weight-gradient, LayerNorm-backward and loss / metric tasks of the level
    void *table_w = nullptr, *table_l = nullptr, *table_m = nullptr;
    int n_w = 0, n_l = 0, tile_w = 0, tile_l = 0, tile_m = 0;
    // host copies of the device task tables above, as schedule() uploaded them (fql_debug_plan, fql_group_s::zip)
    std::vector<GemmTask> h_gemm;
    std::vector<WgradTask> h_wgrad;
    std::vector<LnBwdTask> h_ln;
    std::vector<MiscTask> h_misc;
    bool ka = false;             // OP_GEMM64: the tasks travel as the kernel argument and the tables stay unused (bind_side)
    std::vector<int> waits;      // launches of the OTHER lane that must have completed
    bool record_after = false;   // some launch of the other lane waits on this one
    hipEvent_t ev = nullptr;
};

// FQL_KERNARG_TASKS=0: every launch reads its tasks from its table in HBM (A/B, and the bitwise test of the argument form).  Read when an
// engine is created.
inline bool ka_tasks_env() {
    const char* e = getenv("FQL_KERNARG_TASKS");
    return !e || atoi(e) != 0;
}
// FQL_FUSED_TAIL=0: the FQL update keeps its finalize launch; by default the last-arriving workgroup of its two Adam launches runs that code
// (DESIGN.md section 4).  For the A/B and the bitwise twin of the tests.  Read when an engine is created.
inline bool fused_tail_env() {
    const char* e = getenv("FQL_FUSED_TAIL");
    return !e || atoi(e) != 0;
}
// FQL_AQL_ACQUIRE=1: every kernel packet of every AQL program keeps its agent-scope acquire (the A/B switch and the fallback of build_aql's
// L1-independent programs).  Read when an engine is created.
inline bool aql_acquire_env() {
    const char* e = getenv("FQL_AQL_ACQUIRE");
    return e && atoi(e) != 0;
}
// The kernels that read everything an earlier launch of their program wrote past the L1 and the scalar cache (fql_kernels.h ldx: the audit
// list is FQL_DUMP's "in-update reads"), with the twins that share their bodies.  A program all of whose launches bind one of these needs
// no acquire between its packets (build_aql).  Not here: fql_finalize_kernel (its partials are plain loads: an update with FQL_FUSED_TAIL=0
// keeps its acquires), the convolution family and every other agent kind's kernels.
inline bool l1_independent_kernel(const void* fn) {
#define FQL_L1_CHAIN(HH)                                                                                                                             \
    (const void*)fql_chain_kernel<HH, 0>, (const void*)fql_chain_kernel<HH, 1>, (const void*)fql_chain_kernel<HH, 2>, (const void*)fql_chain_kernel<HH, 3>, \
    (const void*)fql_chain_multi_kernel<HH, 0>, (const void*)fql_chain_multi_kernel<HH, 1>, (const void*)fql_chain_multi_kernel<HH, 2>,             \
    (const void*)fql_chain_multi_kernel<HH, 3>, (const void*)fql_chain_split_kernel<HH, 0>, (const void*)fql_chain_split_kernel<HH, 1>,             \
    (const void*)fql_chain_split_kernel<HH, 2>
    static const void* const table[] = {
        (const void*)fql_prep_kernel, (const void*)fql_prep_multi_kernel,
        (const void*)fql_gemm16_kernel<false>, (const void*)fql_gemm16_kernel<true>,
        (const void*)fql_gemm16_euler_kernel<false>, (const void*)fql_gemm16_euler_kernel<true>,
        (const void*)fql_side_kernel, (const void*)fql_side_ka_kernel, (const void*)fql_side_big_kernel, (const void*)fql_side_big_ka_kernel,
        (const void*)fql_side_split_kernel, (const void*)fql_side_split_ka_kernel,
        FQL_L1_CHAIN(256), FQL_L1_CHAIN(512),
        (const void*)fql_dgrad0_kernel, (const void*)fql_dgrad0_multi_kernel, (const void*)fql_head_dgrad_kernel, (const void*)fql_head_dgrad_multi_kernel,
        (const void*)fql_loss_actor_kernel, (const void*)fql_loss_actor_multi_kernel,
        (const void*)fql_euler_finish_kernel, (const void*)fql_euler_finish_multi_kernel,
        (const void*)fql_adam_kernel, (const void*)fql_adam_multi_kernel, (const void*)fql_wfrag_kernel};
#undef FQL_L1_CHAIN
    for (const void* k : table) if (k == fn) return true;
    return false;
}
// a side-lane launch's four host tables as SideArgs; null when a family exceeds its capacity
inline std::unique_ptr<SideArgs> ka_side_args(const Launch& L) {
    const size_t ng = L.h_gemm.size(), nw = L.h_wgrad.size(), nl = L.h_ln.size(), nm = L.h_misc.size();
    if (ng > FQL_KA_GEMM || nw > FQL_KA_WGRAD || nl > FQL_KA_LN || nm > FQL_KA_MISC) return nullptr;
    auto a = std::make_unique<SideArgs>();
    std::memset(a.get(), 0, sizeof(SideArgs));
    SideFront& f = a->f;
    f.tile_w = L.tile_w; f.tile_l = L.tile_l; f.tile_m = L.tile_m; f.tl = -1;
    for (int& v : f.g0) v = FQL_KA_FRONT_PAD;
    for (int& v : f.w0) v = FQL_KA_FRONT_PAD;
    for (int& v : f.l0) v = FQL_KA_FRONT_PAD;
    for (size_t i = 0; i < ng; ++i) { a->g[i] = L.h_gemm[i]; if (i) f.g0[i - 1] = L.h_gemm[i].tile0; }
    for (size_t i = 0; i < nw; ++i) { a->w[i] = L.h_wgrad[i]; if (i) f.w0[i - 1] = L.h_wgrad[i].tile0; }
    for (size_t i = 0; i < nl; ++i) { a->l[i] = L.h_ln[i]; if (i) f.l0[i - 1] = L.h_ln[i].tile0; }
    for (size_t i = 0; i < nm; ++i) a->m[i] = L.h_misc[i];
    return a;
}
// What an Adam launch does besides its chunks, decided by the program that emits it (fql_engine::adam_for)
struct AdamOpt {
    float lr = 0.f;           // > 0: this launch's learning rate (IQL-diffusion: one per TrainState), else fql_config.lr
    DevState* st = nullptr;   // the counters this launch's bias correction reads (IQL-diffusion's actor), null: the handle's
    int polyak = -1;          // Polyak range in floats from offset 0 (-1: critic_size; 0: no Polyak step)
    bool fin = false;         // an update without a finalize launch: the workgroups take tickets, the last one runs that code
};
struct Program {
    std::vector<Op> ops;
    std::vector<Launch> launches;
    bool lane_used[FQL_LANES] = {};
    hipEvent_t ev_fork = nullptr, ev_join[FQL_LANES] = {};
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int64_t macs = 0;
    AqlProgram aql;            // the program as AQL packets (fql_aql.h): built by its first update on the engine's own stream
    bool aql_tried = false;    // build_aql has run for it (lazily: data-parallel and graph-only users never start the HSA side)
};

// Puts a launch list (a Program's, or an agent group's) onto streams; the only copy of the lane loop.  ls == nullptr: every launch on
// s0 in list order, which is a topological order of the program.  Otherwise lane 0 runs on s0 and lane l >= 1 on ls[l]: a launch first
// waits for the events of the launches in its `waits`, a launch that another lane waits on records its event (created on first use),
// and every used lane >= 1 is joined back into s0 at the end.  fork: those lanes first start behind what s0 holds (else the caller
// orders them).  issue(launch, stream) enqueues one launch.
template <typename P, typename IssueFn>
void issue_lanes(P& pr, hipStream_t s0, const hipStream_t* ls, bool fork, IssueFn&& issue) {
    auto lazy = [](hipEvent_t& e) { if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); };
    bool side = false;   // a lane >= 1 runs on a stream of its own
    if (ls) for (int l = 1; l < FQL_LANES; ++l) side |= pr.lane_used[l];
    if (side && fork) {
        lazy(pr.ev_fork);
        HIP_CHECK(hipEventRecord(pr.ev_fork, s0));
        for (int l = 1; l < FQL_LANES; ++l) if (pr.lane_used[l]) HIP_CHECK(hipStreamWaitEvent(ls[l], pr.ev_fork, 0));
    }
    for (auto& L : pr.launches) {
        const hipStream_t s = side && L.lane != 0 ? ls[L.lane] : s0;
        if (side)
            for (int w : L.waits) if (pr.launches[w].ev) HIP_CHECK(hipStreamWaitEvent(s, pr.launches[w].ev, 0));
        issue(L, s);
        if (side && L.record_after) {
            lazy(L.ev);
            HIP_CHECK(hipEventRecord(L.ev, s));
        }
    }
    if (side)
        for (int l = 1; l < FQL_LANES; ++l) {
            if (!pr.lane_used[l]) continue;
            lazy(pr.ev_join[l]);
            HIP_CHECK(hipEventRecord(pr.ev_join[l], ls[l]));
            HIP_CHECK(hipStreamWaitEvent(s0, pr.ev_join[l], 0));
        }
    HIP_CHECK(hipGetLastError());
}
// the events issue_lanes created for a launch list
template <typename P>
void destroy_lane_events(P& pr) {
    for (auto& L : pr.launches) if (L.ev) { hipEventDestroy(L.ev); L.ev = nullptr; }
    if (pr.ev_fork) { hipEventDestroy(pr.ev_fork); pr.ev_fork = nullptr; }
    for (hipEvent_t& e : pr.ev_join) if (e) { hipEventDestroy(e); e = nullptr; }
}

// what `body` enqueues on `s` (and on the streams it forks from `s`) as an instantiated graph; a body that throws ends the capture first
template <typename Body>
void capture_graph(hipStream_t s, Body&& body, hipGraph_t& graph, hipGraphExec_t& exec) {
    static const bool trace = getenv("FQL_TRACE") != nullptr;
    HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    try {
        body();
    } catch (...) {
        hipGraph_t g = nullptr;
        hipStreamEndCapture(s, &g);
        if (g) hipGraphDestroy(g);
        throw;
    }
    if (trace) fprintf(stderr, "[fql] end capture\n");
    HIP_CHECK(hipStreamEndCapture(s, &graph));
    if (trace) {
        size_t nn = 0;
        hipGraphGetNodes(graph, nullptr, &nn);
        fprintf(stderr, "[fql] instantiate (%zu nodes)\n", nn);
    }
    HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    if (trace) fprintf(stderr, "[fql] instantiated\n");
}

// Every update program holds its captured graph once build_workspace has returned: only a rebuild that failed halfway (and freed the
// old programs) leaves one without.  The update entry points report that instead of launching a null graph.
void require_graph(const Program& pr) {
    if (!pr.exec) throw HipError{"no update program: the last workspace rebuild (fql_set_batch_size) failed halfway"};
}

struct PassBuf {
    int net = 0, M = 0;
    const void* id = nullptr;          // dependency id base
    float* x0 = nullptr;               // [M, in_p]
    std::vector<float*> g, xn, z, stats;  // per hidden layer
    std::vector<float*> lnpart;        // LN layers: per-row partial sums per 32 columns (LDS-tiled kernels)
    float* out = nullptr;              // [M, out_p]
    std::vector<float*> dz;            // per layer gradient wrt pre-activation / output
    std::vector<float*> dy;            // LN nets: gradient wrt LN output
    float* dx0 = nullptr;
};

// activations of one encoder pass over n images (kept for the backward pass)
struct EncBuf {
    int enc = 0, n = 0;
    const unsigned char* img = nullptr;
    struct St { float *c0 = nullptr, *pool = nullptr; unsigned char* arg = nullptr; std::vector<float*> c1, y; };
    std::vector<St> st;
    float *frelu = nullptr, *z = nullptr, *E = nullptr;   // [n, flat], [n, enc_dim] x 2
    // backward scratch (allocated only for differentiated passes)
    float *dz = nullptr, *dA = nullptr, *dB = nullptr, *dC = nullptr;
    std::map<const void*, float*> wpart;   // per convolution (keyed by its arena weight pointer): weight-gradient partials, so the
                                            // wgrads of a pass are independent and their folds share launches
    std::map<const void*, size_t> bytes;   // allocated size of every activation / scratch buffer above (fql_debug_enc's bound)
};

// ------------------------------------------------------------------------------------------------
// agent kinds: what a handle is, and what the engine says about it
// ------------------------------------------------------------------------------------------------
enum class AgentKind { FQL, IFQL, REBRAC, SAC, BC, IQL, IQLD, CFGRL };
constexpr int kNumKinds = 8;

const char* const k_info_names[FQL_NUM_INFO] = {
    "critic/critic_loss", "critic/q_mean", "critic/q_max", "critic/q_min", "actor/actor_loss",
    "actor/bc_flow_loss", "actor/distill_loss", "actor/q_loss", "actor/q", "actor/mse",
    "grad/max", "grad/min", "grad/norm"};
const char* const k_ifql_info_names[FQL_IFQL_NUM_INFO] = {
    "value/value_loss", "value/v_mean", "value/v_max", "value/v_min", "critic/critic_loss", "critic/q_mean", "critic/q_max",
    "critic/q_min", "actor/actor_loss", "grad/max", "grad/min", "grad/norm"};
const char* const k_rebrac_info_names[FQL_REBRAC_NUM_INFO] = {
    "critic/critic_loss", "critic/q_mean", "critic/q_max", "critic/q_min", "actor/total_loss", "actor/actor_loss", "actor/bc_loss",
    "actor/std", "actor/mse", "grad/max", "grad/min", "grad/norm"};
const char* const k_sac_info_names[FQL_SAC_NUM_INFO] = {
    "critic/critic_loss", "critic/q_mean", "critic/q_max", "critic/q_min", "actor/total_loss", "actor/actor_loss", "actor/alpha_loss",
    "actor/alpha", "actor/entropy", "actor/std", "actor/q", "grad/max", "grad/min", "grad/norm"};
const char* const k_bc_info_names[FQL_BC_NUM_INFO] = {"bc_loss", "grad/max", "grad/min", "grad/norm"};
const char* const k_iql_info_names[2][FQL_IQL_DDPGBC_NUM_INFO] = {
    {"value/value_loss", "value/v_mean", "value/v_max", "value/v_min", "critic/critic_loss", "critic/q_mean", "critic/q_max", "critic/q_min",
     "actor/actor_loss", "actor/adv", "actor/bc_log_prob", "actor/mse", "actor/std", "grad/max", "grad/min", "grad/norm", nullptr, nullptr, nullptr},
    {"value/value_loss", "value/v_mean", "value/v_max", "value/v_min", "critic/critic_loss", "critic/q_mean", "critic/q_max", "critic/q_min",
     "actor/actor_loss", "actor/q_loss", "actor/bc_loss", "actor/q_mean", "actor/q_abs_mean", "actor/bc_log_prob", "actor/mse", "actor/std",
     "grad/max", "grad/min", "grad/norm"}};
const char* const k_iqld_info_names[FQL_IQLD_NUM_INFO] = {
    "critic_loss", "q", "value_loss", "v", "v_min", "v_max", "actor_q", "actor_loss", "actor_positive_ratio", "actor_loss_positive",
    "actor_loss_uncond", "o_mean", "o_std", "o_min", "o_max", "effective_batch_size", "loss_weights_top_10_mass", "loss_weights_max",
    "grad/max", "grad/min", "grad/norm"};
const char* const k_cfgrl_info_names[FQL_CFGRL_NUM_INFO] = {"actor/actor_loss", "grad/max", "grad/min", "grad/norm"};

enum { NZ_EPS1 = 1, NZ_X0 = 2, NZ_T = 4, NZ_Z = 8, NZ_EPS2 = 16 };   // the fields of fql_noise

// What a kind's row is made of (KindDesc, below).
// A module of the parameter tree: its nets (n1 >= 0: the stacked pair), whether it trains, its encoder on a visual handle.  n0 < 0: a
// module without a net (SAC's 0-d LogParam).  actor: an Actor module, whose last layer is read back as mean_net behind actor_net.
struct Mod { const char* name; const char* sub; int n0, n1; bool train; int enc; bool actor = false; };
// Where a kind's special leaves sort among the generic ones (KindDesc::special_leaves is called at each of these places)
enum LeafSite { LS_BARE_HEAD, LS_NO_NET, LS_ACTOR_HEAD, LS_LAST };   // behind a bare net's Dense_0; a module without a net; behind an Actor's actor_net; behind every module
enum HeadInit { HI_GLOROT, HI_LECUN_TRUNC, HI_TWO_HEADS };   // the actor head's initialiser (init_params)
struct EmbedInit { int n, fan_in; };                          // the embedding at emb_off: n floats of the untruncated N(0, 1 / fan_in)
struct InfoSet { const char* const* names; int n; };
enum Sampler { SMP_ONESTEP, SMP_BEST_OF_N, SMP_ACTOR, SMP_FLOW };   // sample_actions: FQL's one-step actor, IFQL's best of N, an actor on obs, a flow policy
// One chunk of an actor kind's sampling call behind the actor's forward: mean [m, out_p] -> out [m, act]; z: the caller's noise or null
struct ActChunk { const float *mean, *z; float* out; uint64_t sd; int m, start; float temperature; };
// What differs between the hoisted flow samplers (DESIGN.md sections 16 and 18-20): BC's, and the two CFG kinds' with a scalar cfg
// or, as a sweep, with one guidance weight per row.  A row holds halves, shared_x and tables; flow_shape() fills in the handle's rest.
struct FlowShape {
    int halves;      // 1: BC, one block of n_pad rows.  2: the CFG kinds, rows [0, half) the positive / conditional pass, [half, n_pad) the unconditional one
    bool shared_x;   // the halves share X = [obs | 0] and C0 (IQL-diffusion); CFGRL's differ in the goal columns
    int tables;      // step-bias rows per step: 1 BC [S, H], 2 IQL-diffusion [S, 2, H], 0 CFGRL (t is an argument of its layer-0 kernels)
    int S;           // Euler steps
    int goal_dim;    // CFGRL: the goal block in front of the action rows of W0, and goals to stage; else 0
    bool sweep;      // the weights come per row from the workspace (cfgs), and the combine of step i - 1 rides in front of layer 0 of step i
};
// A module a handle answers for in fql_module_forward, under the reference's name without "modules_".  members 2: the stacked critic,
// nets `net` and `net + 1` on the same rows.  scalar: the head is one column (Value), the result [members, n]; else [n, act].
struct ModuleSpec { const char* name; int net, members; bool scalar, act, times; };
enum : unsigned {   // traits of a kind
    K_CRITIC = 1,         // a critic pair and its target (NET_C0..NET_T1)
    K_OWN_INFO = 2,       // the infos live in iql_info, not in DevState::info
    K_POLYAK_ALL = 4,     // Polyak moves the whole trained range: critic_size = n_train (rebrac.py:131-133: critic pair and actor)
    K_CHAIN = 8,          // the Euler-chain kernel is admitted (build_chain_weights)
    K_TIME_TABLE = 16,    // the timestep-embedding table d_emb; an explicit t is read on the grid {0, 1/S, ..., 1}
    K_NEXT_ACTIONS = 32,  // update_from_dataset takes next_actions from the dataset (utils/datasets.py:96-100)
    K_ACTOR_STATE = 64,   // a second DevState, d_state_a: the actor TrainState's own counters
    K_GOALS = 128,        // a goal source (d_gsrc), a goal block in the actor's rows; the goal config holds the sampler's steps
    K_VISUAL = 256,       // visual encoders and the bf16 x 3 precision are available
};
// One row per kind, indexed by AgentKind: everything the single-handle layer decides by the kind.  The table, k_kinds, stands behind
// fql_engine, whose members its rows name.  A new agent adds an enumerator, a row and its hooks there, and a column to EP_TABLE (C ABI).
struct KindDesc {
    const char* name;               // "IFQL": create-time messages
    const char* label;              // "an IFQL handle": entry-point messages
    const char* create;             // its create call
    unsigned traits;                // K_*
    const char* const* info_names;
    int num_info;
    InfoSet (*infos)(const fql_engine&);   // where names and count depend on the handle's config (IQL: by actor_loss); else null
    int probe_infos, probe_terms[3];       // fql_total_loss: the infos it returns, the info slots whose sum is the loss (-1: none)
    int noise_reads;                // NZ_* fields of fql_noise the kind reads; any other must be NULL ...
    const char* noise_refusal;      // ... or fill_noise refuses with this
    // create: the refusal of a kind config or null; the copy of the config into the engine
    const char* (*check)(const void* kind_cfg);
    void (*adopt)(fql_engine&, const void* kind_cfg);
    // the arena: NET_BC / NET_OS / NET_TA over (obs, act) widths; the trained floats a kind keeps behind NET_OS and the member that holds their offset
    void (*nets)(fql_engine&, int od, int ad);
    size_t fql_engine::* extra_off;
    size_t (*extra_floats)(const fql_engine&);
    // leaves: the modules in the parameter tree's order, the prefix of a bare policy net's leaves (null: none), the prefixes of the three
    // trained modules in chunk order (all null: one module, every chunk), the kind's special leaves (returns true where it wrote an Actor's heads itself)
    const Mod* mods;
    int nmods;
    const char* bare;
    const char* trained[3];
    bool (*special_leaves)(fql_engine&, LeafSite, const Mod*);
    // initialisers: the actor head's, the Glorot scale of HI_GLOROT / HI_TWO_HEADS (null: 1), the embedding's (null: none)
    HeadInit head_init;
    double (*head_scale)(const fql_engine&);
    EmbedInit (*embed_init)(const fql_engine&);
    // per batch size: the update workspace and programs; the multiply-accumulates of one update
    void (fql_engine::*workspace)();
    int64_t (*macs)(const fql_engine&);
    // sampling and queries: the sampler; SMP_ACTOR: the launch behind the actor's forward; SMP_FLOW: halves, shared_x, tables; fql_module_forward's modules
    Sampler sampler;
    void (*act)(const fql_engine&, const ActChunk&, hipStream_t);
    FlowShape flow;
    const ModuleSpec* modules;
    int nmodules;
};

}  // namespace

struct fql_group_s;
struct fql_engine {
    fql_config cfg{};
    AgentKind kind = AgentKind::FQL;
    const KindDesc& desc() const;
    bool has(unsigned trait) const { return (desc().traits & trait) != 0; }
    bool actor_on_obs() const { return desc().sampler == SMP_ACTOR; }   // NET_BC is actor(obs), no flow
    bool flow_sampler() const { return desc().sampler == SMP_FLOW; }
    bool own_info() const { return has(K_OWN_INFO); }
    InfoSet infos() const { return desc().infos ? desc().infos(*this) : InfoSet{desc().info_names, desc().num_info}; }
    int num_info() const { return infos().n; }
    const char* const* info_names() const { return infos().names; }
    // IFQL agent (agents/ifql.py; fql_ifql_create): the arena's NET_OS slot holds the value net (obs -> 1, LayerNorm like the critic),
    // NET_BC is actor_flow; critic, target and their place in the arena are FQL's.  The update is build_ifql_program.
    float expectile = 0.9f;
    int num_samples = 32;
    float* X_v = nullptr;   // [2B, value in_p]: [obs ; next_obs]
    PassBuf p_v;            // value pass over X_v (backward over the obs half only)
    // ReBRAC agent (agents/rebrac.py; fql_rebrac_create): NET_BC holds the actor (obs -> mean), NET_OS is empty and NET_TA, the target
    // actor, follows the target critic, so the Polyak range [0, critic_size = n_train) of fql_adam_kernel covers critic and actor.
    // Two update programs: prog_full (full_update=True) and prog_critic (critic-only step: no actor passes, zero actor gradient, no Polyak).
    fql_rebrac_config rcfg{};
    float *X_a = nullptr, *X_ta = nullptr, *X_t = nullptr, *X_q = nullptr;   // actor inputs [B, inp_a] (obs, next_obs); critic inputs [B, inp_c]
    float *w_nact = nullptr, *w_noise = nullptr;                            // [B, ap]: next_actions, raw N(0, 1) of the target-policy noise
    PassBuf p_a, p_ta, p_q[2];                                               // actor, target actor, critic pair on [obs | actor actions]
    Program prog_critic;
    // SAC agent (agents/sac.py; fql_sac_create): NET_BC holds the actor, whose last layer is both heads as one [H, 2 ap] layer (mean
    // columns [0, ap), raw log-std [ap, 2 ap)); modules_alpha/log_value sits in the NET_OS slot (4 floats at alpha_off), so the trained
    // region is critic pair, actor, log_value and the Polyak range [0, critic_size) is the critic pair's.  p_a runs over X_a = [obs ;
    // next_obs] (2B rows; backward over the obs rows), p_q[] is the critic pair on [obs | a], p_ct[] the target pair on [next_obs | a'].
    fql_sac_config scfg{};
    float target_entropy = 0.f;
    size_t alpha_off = 0;
    float *w_eps = nullptr, *lp_buf = nullptr;   // [2B, ap]: eps_c rows then eps_n rows; [2B]: log-probabilities of a, then of a'
    // BC agent (agents/bc.py; fql_bc_create): the arena holds ONE net, the policy, in the NET_BC slot (input [obs | x_t | emb(t)], every
    // other net is empty, so critic_size = 0 and Adam has no Polyak range).  One lane: prep, forward, loss, backward, Adam, finalize.
    int bc_steps = 16;            // denoise_steps S
    float* d_emb = nullptr;       // [(S + 1), 16] timestep-embedding table (built on the host at create)
    bool lane0_64 = false;        // while the BC update program is built: lane 0 takes the 64-column LDS-tiled kernels and keeps its weight gradients
    // IQL agent (agents/iql.py; fql_iql_create): NET_OS holds the value net and the critic pair and its target sit where IFQL's do; NET_BC
    // is the Gaussian actor (actor_net + mean_net, obs -> act) and modules_actor/log_stds ([act], const_std = 0 only) follows the value
    // net at ls_off, padded to ap floats.  p_v, p_c1[], p_ct[] as IFQL's; p_a is the actor on obs; ddpgbc adds p_q[], the critic pair on
    // [obs | q_actions].  The infos (16 or 19) live in iql_info: [0, 32) of the last update, [32, 64) of the last loss probe.
    fql_iql_config qcfg{};
    size_t ls_off = 0;
    float *se_buf = nullptr, *ls_part = nullptr;   // [B]: squared error per row; [B, ap]: per-row terms of the log_stds gradient
    float* iql_info = nullptr;
    // IQL-diffusion agent (agents/iql_diffusion.py, binary optimality family; fql_iqld_create): critic pair, target pair and value net as
    // IQL's; NET_BC is the DiffusionPolicy on [obs | x_t | emb(t) | Embed[is_positive]] (BC's policy with 32 more input columns) and
    // Embed_0/embedding ([2, 32]) follows the value net at emb_off.  p_bc runs over 2B rows (positive half, unconditional half).  Four
    // programs on one handle: prog_full (both), prog_critic (critic and value only), prog_actor (actor only), prog_none (neither: the RNG
    // step alone).  The critic and the value TrainState count in d_state, the actor's in d_state_a.  The 21 infos live in iql_info ([0, 32)
    // of the last update, [32, 64) of the last loss probe), the three per-row arrays in rows_buf ([2][3][B], the same halves).
    fql_iqld_config dcfg{};
    size_t emb_off = 0;
    DevState* d_state_a = nullptr;
    float *w_lw = nullptr, *rows_buf = nullptr;   // [B] loss weights; [2][3][B]
    Program prog_actor, prog_none;
    float sample_cfg = 1.0f;                      // cfg of the sampling call in flight (read when its step launches are issued)
    // CFGRL agent (agents/cfgrl.py; fql_cfgrl_create): the arena holds actor_flow in the NET_BC slot (input [obs | goal | x_t | t]) and
    // modules_unc_embed/Embed_0/embedding ([1, G], padded to 16 floats) behind it at emb_off; every other net is empty, so critic_size = 0
    // and Adam has no Polyak range, as on a BC handle.  One lane: prep, forward, loss, backward, embedding gradient, Adam, finalize.
    // Where a step's goals and mask come from travels in d_gsrc (CfgrlSrc), rewritten only when it changes, as d_src is.  The goal draw of
    // update_from_dataset reads ds_final / ds_reps (fql_cfgrl_dataset_goals).  The per-row read-back (cf_rows, cf_draws, cf_mask) has two
    // halves: the last update's, then the last loss probe's.
    fql_cfgrl_config gcfg{};
    CfgrlSrc* d_gsrc = nullptr;
    CfgrlSrc* h_gsrc_ring = nullptr;
    CfgrlSrc h_gsrc_shadow{};
    bool gsrc_valid = false;
    int gsrc_ring_pos = 0;
    int64_t* ds_final = nullptr;
    float* ds_reps = nullptr;
    float* in_goal = nullptr;                     // [B, G] staging of host goals
    unsigned char *in_cfg = nullptr, *cf_mask = nullptr;   // [B] staging of a host mask; [2][B] do_cfg
    int64_t* cf_rows = nullptr;                   // [2][2][B]
    uint32_t* cf_draws = nullptr;                 // [2][CFGRL_NUM_DRAWS][B]
    uint64_t seed = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t lane_streams[FQL_LANES] = {};   // lanes >= 1 of the engine's programs (lane 0 runs on the stream a program is issued on)
    bool allow64 = true;
    int emit_lane = 0;
    std::vector<Op>* defer_wgrads = nullptr;   // when set, emit_backward collects weight-gradient ops here instead of emitting them in place
    std::string err;

    Net nets[NUM_NETS];
    EncNet encs[NUM_ENC];
    ConvWprepTask* enc_wprep[NUM_ENC] = {nullptr, nullptr, nullptr, nullptr};   // device task tables of fql_conv_wprep_kernel
    int enc_nconv[NUM_ENC] = {0, 0, 0, 0};
    std::vector<void*> enc_allocs;
    bool visual = false;
    int enc_dim = 0;
    unsigned char* img_all = nullptr;   // [2B] images: obs batch, then next_obs batch (fixed address: graphs bake it in)
    EncBuf eb_c, eb_t, eb_bc, eb_os;
    size_t n_train = 0, n_total = 0, critic_size = 0;
    float *P = nullptr, *G = nullptr, *Mu = nullptr, *Nu = nullptr;
    std::vector<Leaf> leaves;
    int n_train_leaves = 0;
    AdamChunk* d_chunks = nullptr;
    float* d_partials = nullptr;
    int* d_leaf_range = nullptr;
    int n_chunks = 0;

    DevState* d_state = nullptr;
    SrcDesc* d_src = nullptr;
    SrcDesc h_src_shadow{};
    bool src_valid = false;
    SrcDesc* h_src_ring = nullptr;
    int src_ring_pos = 0;

    // workspace (per batch size)
    int B = 0;
    std::vector<void*> ws_allocs;
    float *in_obs = nullptr, *in_act = nullptr, *in_rew = nullptr, *in_mask = nullptr, *in_nobs = nullptr, *in_nact = nullptr;
    float* in_noise[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t* in_idx = nullptr;
    float *X_os = nullptr, *X_bc = nullptr, *X_eu = nullptr, *X_c1 = nullptr, *X_c2 = nullptr, *X_ct = nullptr;
    float *vel = nullptr, *w_rew = nullptr, *w_mask = nullptr, *w_act = nullptr, *tgt = nullptr;
    float *X_e0 = nullptr, *C0 = nullptr, *Abuf[2] = {nullptr, nullptr}, *Vpart = nullptr;  // fused Euler chain
    bool fused_euler = false;
    // Euler-chain kernel (fql_chain.h): fragment-major copies of the BC flow's hidden kernels (layers 1..nh-1), of the 16 rows of
    // W0 that start at the action block and of the head kernel, refreshed behind every Adam step of that module
    bool use_chain = false;
    int fill_lane_full = 1;          // lane of the critic-loss / BC passes (and of their Adam launches) in the single-GPU programs
    std::vector<float*> wf_bc;       // per layer 1..nh-1: [H/4][H][4]
    float *wf_w0 = nullptr, *wf_w4 = nullptr;
    WfragTask* d_wfrag = nullptr;
    std::vector<WfragTask> h_wfrag;   // host copy of d_wfrag (fql_group_s::zip)
    int wfrag_n = 0, wfrag_grid = 0;
    const bool ka_tasks = ka_tasks_env();   // FQL_KERNARG_TASKS, as it stood when this engine was created
    const bool fused_tail = fused_tail_env();   // FQL_FUSED_TAIL, as it stood when this engine was created
    unsigned* d_ticket = nullptr;    // arrival counter of an update's Adam workgroups (fql_adam_body): 0 between updates
    std::vector<void*> chain_allocs;
    bool split_build = false;   // building the data-parallel program: lane 1 must not depend on lane 0's backward
    bool wide_tiles = false;    // three-lane programs: 32 x 64 side tiles everywhere (the other lanes fill the CUs a launch leaves idle; +1 %)
    bool split_ok = false;
    int vp_tiles = 0;
    int num_cus = 0;
    PassBuf p_os, p_os_bwd, p_bc, p_eu, p_c1[2], p_c2[2], p_ct[2];
    Program prog_fwdbwd, prog_opt, prog_loss;
    Program prog_opt_split;   // the optimizer half with the critic's / BC flow's Adam on lane 1: fql_update_end_split issues that lane on the stream that carried bucket 0's all-reduce
    Program prog_full;   // single-GPU update in ONE graph: per-module Adam launches start as soon as that module's gradients exist
    int mod_chunk0[3] = {0, 0, 0}, mod_chunkn[3] = {0, 0, 0};  // chunk ranges of bc_flow, onestep, critic (leaf order)
    // data-parallel variant: the same update as three single-lane graphs (lane 0 before / after it needs lane 1, lane 1)
    // so the gradient bucket of lane 1 can be all-reduced while lane 0 is still running
    Program prog_split;
    hipGraphExec_t split_exec[4] = {nullptr, nullptr, nullptr, nullptr};  // A0 (prep), B (lane 1), A1, A2
    hipGraph_t split_graph[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;
    bool split_begun = false;   // the pending update was begun by launch_split (ev_c marks the end of lane 0's pre-join part)
    bool began = false;
    // the single-GPU update as AQL packets on the engine's own HSA queues (fql_aql.h); everything else stays on HIP streams
    AqlRuntime aql;
    bool last_update_aql = false;
    bool hip_dirty = true;                         // HIP work may be pending on the engine's stream: drain it before the next AQL submit
    void aql_drain() {                             // every AQL update submitted so far has finished (host wait)
        if (!aql.up) return;
        try { aql.drain(); } catch (const AqlError& e) { throw HipError{e.msg}; }
    }

    // dataset
    float *ds_obs = nullptr, *ds_act = nullptr, *ds_rew = nullptr, *ds_mask = nullptr, *ds_nobs = nullptr;
    float* ds_row = nullptr;
    int64_t ds_size = 0, ds_cap = 0, ds_ptr = 0;
    // frames dataset (visual agents): uint8 frames + per-row episode start, frame stacking and crop done by the gather
    unsigned char *ds_frames = nullptr, *ds_next_frames = nullptr;
    int64_t* ds_init = nullptr;
    int ds_fs = 0;
    float ds_paug = 0.f;
    // replay ring beside the training dataset (balanced sampling, main.py:106-109,255-259): same row layout, starts empty
    float *rb_obs = nullptr, *rb_act = nullptr, *rb_rew = nullptr, *rb_mask = nullptr, *rb_nobs = nullptr;
    unsigned char *rb_frames = nullptr, *rb_next_frames = nullptr;
    int64_t* rb_init = nullptr;
    int64_t rb_size = 0, rb_cap = 0, rb_ptr = 0;
    int64_t* in_init = nullptr;   // [B] workspace
    int *in_crop = nullptr, *in_crop_user = nullptr;  // [B][2]

    // eval (sample_actions / flow_actions) workspaces keyed by padded row count
    struct Eval {
        int n_pad = 0;
        std::vector<void*> allocs;
        float *X = nullptr, *Xf = nullptr, *tgt = nullptr;
        PassBuf p_os, p_eu;
        Program prog_os, prog_flow;
        float *st_obs = nullptr, *st_noise = nullptr, *st_out = nullptr;
        float* st_goal = nullptr;   // CFGRL: staging of host goals [half, G]
        float *Xf2 = nullptr, *cfgs = nullptr;   // sweep programs: the second ping-pong buffer of x [half, ap]; the per-row weights [half]
        // visual agents: the rows are images; they pass through the module's encoder first (agents/fql.py:162-163, networks.py:221)
        unsigned char* st_img = nullptr;
        EncBuf eb_os, eb_bc;
        Program prog_enc_os, prog_enc_bc;
        // IFQL best-of-N: the critic pair on [obs | clip(flow action)] of every sample row
        float* Xq = nullptr;
        PassBuf p_q[2];
        Program prog_q;
    };
    // (the bool: the sweep programs of the CFG samplers, workspaces of their own: get_eval)
    std::map<std::pair<int, bool>, std::unique_ptr<Eval>> evals;
    // module queries (fql_module_forward): the workspace of one module's forward over n_pad padded rows, keyed by (index in modules(),
    // n_pad).  Buffers and program are its own: no update, loss-probe or sampling workspace is read or written by a query.
    struct Query {
        std::vector<void*> allocs;
        float* X = nullptr;        // [n_pad, in_p]: [obs | act | t | 0]
        PassBuf p[2];              // one pass per member (the critic pairs: two nets on the same X)
        Program prog;
        float *st_obs = nullptr, *st_act = nullptr, *st_t = nullptr, *st_out = nullptr;   // staging of host rows / of a host result
    };
    std::map<std::pair<int, int>, std::unique_ptr<Query>> queries;

    // agent groups (fql_group_*): the group this engine is a member of, the event behind that group's last update and whether an entry
    // point of this engine has run since (then the next group update orders itself behind this engine's stream)
    fql_group_s* group = nullptr;
    hipEvent_t grp_done = nullptr;
    bool grp_pending = false, grp_touched = true;
    // grp_legacy: that update ran on the legacy default stream (FQL_STREAM_LEGACY).  No event is recorded there: the HIP runtime keeps the
    // stream's handle, (hipStream_t)1, in the event, and hipStreamWaitEvent on such an event dereferences it.  Waiting for such an update
    // is a device synchronise instead.
    bool grp_legacy = false;
    void group_fence() {   // host wait for the group's last update (every entry point: it may read or write what that update writes)
        grp_touched = true;
        if (grp_pending) { HIP_CHECK(grp_legacy ? hipDeviceSynchronize() : hipEventSynchronize(grp_done)); grp_pending = false; }
    }
    void group_order(hipStream_t s) {   // the same as a stream dependency, for entry points that only enqueue on `s`
        grp_touched = true;
        if (!grp_pending) return;
        if (!grp_legacy) HIP_CHECK(hipStreamWaitEvent(s, grp_done, 0));
        else if (s != hipStreamLegacy) { HIP_CHECK(hipDeviceSynchronize()); grp_pending = false; }   // (on the legacy stream itself: in order)
    }
    // lazily read infos (the reference returns device scalars that are only read at log time, main.py:276): a ring of pinned host
    // slots, one asynchronous 52-byte copy + event per ticket
    static constexpr int kInfoRing = 64;
    float (*h_info_ring)[32] = nullptr;
    hipEvent_t info_ev[kInfoRing] = {};
    uint64_t info_seq = 0;

    // ---------------------------------------------------------------------------------------
    float* dalloc(std::vector<void*>& owner, size_t nfloats) {
        void* p = nullptr;
        const size_t bytes = std::max<size_t>(nfloats, 4) * sizeof(float);
        HIP_CHECK(hipMalloc(&p, bytes));
        HIP_CHECK(hipMemset(p, 0, bytes));
        owner.push_back(p);
        return (float*)p;
    }

    static Net make_net(int in, const int32_t* hid, int nh, int out, bool ln) {
        Net n;
        int prev = in;
        for (int i = 0; i <= nh; ++i) {
            Layer L{};
            L.in = prev;
            L.out = (i < nh) ? hid[i] : out;
            L.in_p = (i == 0) ? ((L.in + 63) & ~63) : pad16(L.in);
            L.out_p = pad16(L.out);
            L.ln = ln && i < nh;
            n.layers.push_back(L);
            prev = L.out;
        }
        return n;
    }
    Net actor_net(int in, int out) const { return make_net(in, cfg.actor_hidden, cfg.num_actor_hidden, out, cfg.actor_layer_norm != 0); }
    Net value_net(int in) const { return make_net(in, cfg.value_hidden, cfg.num_value_hidden, 1, cfg.layer_norm != 0); }
    void build_nets() {
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        const KindDesc& kd = desc();
        for (Net& n : nets) n = Net{};
        if (has(K_CRITIC)) nets[NET_C0] = value_net(od + ad);
        kd.nets(*this, od, ad);
        nets[NET_C1] = nets[NET_T0] = nets[NET_T1] = nets[NET_C0];
        size_t off = 0;
        auto place_enc = [&](int ei) {
            if (!visual) return;
            EncNet& en = encs[ei];
            en = EncNet{};
            en.off = off;
            const int sizes[3] = {16, 32, 32};  // impala_small: stack_sizes (16, 32, 32), num_blocks 1 (utils/encoders.py:66-67,106)
            int H = cfg.img_h, W = cfg.img_w, cin = cfg.img_c;
            for (int s = 0; s < 3; ++s) {
                EncStack st;
                st.H = H; st.W = W;
                const int nconv = 1 + 2 * (cfg.encoder == 2 ? 2 : 1);   // impala: num_blocks 2, impala_small: 1 (utils/encoders.py:67,106)
                for (int j = 0; j < nconv; ++j) {
                    ConvL c{};
                    c.cin = cin; c.cout = sizes[s];
                    c.w = off; off += (size_t)9 * c.cin * c.cout;
                    c.b = off; off += c.cout;
                    st.conv.push_back(c);
                    cin = sizes[s];
                }
                en.stacks.push_back(st);
                H /= 2; W /= 2;
            }
            en.flat = H * W * cin;
            Layer& D = en.dense;
            D = Layer{};
            D.in = D.in_p = en.flat; D.out = D.out_p = enc_dim; D.ln = false;
            D.w = off; off += (size_t)D.in_p * D.out_p;
            D.b = off; off += D.out_p;
            en.size = off - en.off;
        };
        for (int ni = 0; ni < NUM_NETS; ++ni) {
            Net& n = nets[ni];
            n.off = off;
            for (Layer& L : n.layers) {
                L.w = off; off += (size_t)L.in_p * L.out_p;
                L.b = off; off += L.out_p;
                if (L.ln) {
                    L.g = off; off += L.out_p;
                    L.be = off; off += L.out_p;
                }
            }
            n.size = off - n.off;
            // every module's encoder follows its MLP(s); the critic's sits inside the Polyak-averaged region
            if (ni == NET_C1) { place_enc(ENC_C); critic_size = off; }
            if (ni == NET_BC) place_enc(ENC_BC);
            if (ni == NET_OS) {
                place_enc(ENC_OS);
                if (const size_t extra = kd.extra_off ? kd.extra_floats(*this) : 0) { this->*kd.extra_off = off; off += extra; }
                n_train = off;
            }
            if (ni == NET_T1) place_enc(ENC_T);
        }
        n_total = off;
        if (has(K_POLYAK_ALL)) critic_size = n_train;
        for (int ni = 0; ni < NUM_NETS; ++ni)
            for (const Layer& L : nets[ni].layers)
                if (L.in_p > 1024 || L.out_p > 1024) invalid("layer widths above 1024 are not supported (got %d -> %d)", L.in, L.out);
        if (nets[NET_T0].off - n_train != 0 || nets[NET_T0].size + nets[NET_T1].size + nets[NET_TA].size + (visual ? encs[ENC_T].size : 0) != critic_size)
            invalid("internal: target arena layout mismatch");
    }

    // can the first convolution of a stack run fused with the stack's max-pool (fql_conv3x3_pool_kernel)?  first_stack: it reads the uint8 images
    // Measured (visual update, one box): the uint8 layer fused +2.8 % (fp32) and more in bf16x3; the float layers of stacks 1 / 2 fused too: bf16x3 370.5 -> 373.9, fp32
    // 311.7 -> 308.3 (their 5-row tiles redo a quarter of the rows, which fp32 MFMAs pay for) - so those are fused under precision = 2 only.
    bool pool_fusable(const EncStack& st, const ConvL& c, bool first_stack) const {
        const int Ci = pad16c(c.cin);
        if (st.W % 16 || st.W < 16 || st.W > 128 || st.H % 2 || (c.cout != 16 && c.cout != 32)) return false;
        if ((size_t)FQL_CONV_POOL_LDS_FLOATS(st.W, Ci, c.cout) * sizeof(float) > 65536) return false;
        if (first_stack) return c.cout == 16 && Ci == 16 && 7 * st.W * c.cin <= 4 * 4 * FQL_THREADS && (st.W * c.cin) % 4 == 0;   // seven uint8 rows: <= 4 dwords per thread
        return cfg.precision == 2 && (Ci == 16 || Ci == 32) && Ci == c.cin && 7 * (st.W + 2) * (Ci / 4) <= 4 * FQL_THREADS;               // seven float rows: <= 4 float4 per thread
    }
    // LDS-layout weight copies of every convolution + the task tables of fql_conv_wprep_kernel (needs P)
    void build_enc_weights() {
        if (!visual) return;
        for (int ei = 0; ei < NUM_ENC; ++ei) {
            std::vector<ConvWprepTask> tasks;
            bool first = true;
            for (EncStack& st : encs[ei].stacks)
                for (ConvL& c : st.conv) {
                    const int Ci = pad16c(c.cin);
                    const bool first_stack = &st == &encs[ei].stacks[0];
                    // precision = 2: the float convolutions read pre-split bf16 hi / lo planes (slightly larger than the fp32 image)
                    const bool split = cfg.precision == 2 && !first && (Ci == 16 || Ci == 32) && (c.cout == 16 || c.cout == 32);
                    // a stack's first convolution runs fused with the stack's max-pool and splits its fragments in registers: its forward copy stays fp32
                    c.pool_fused = (&c == &st.conv[0]) && pool_fusable(st, c, first_stack);
                    c.Wf = dalloc(enc_allocs, std::max((size_t)c.cout * (9 * Ci + 4), (size_t)2 * c.cout * (9 * Ci / 2 + Ci / 4)));
                    c.Wb = first ? nullptr : dalloc(enc_allocs, std::max((size_t)c.cin * (9 * c.cout + 4), (size_t)2 * c.cin * (9 * c.cout / 2 + c.cout / 4)));   // no gradient into the images
                    c.split = split;
                    tasks.push_back(ConvWprepTask{P + c.w, c.Wf, c.Wb, c.cin, c.cout, Ci, split ? (c.pool_fused ? 2 : 1) : 0});
                    first = false;
                }
            enc_nconv[ei] = (int)tasks.size();
            enc_wprep[ei] = (ConvWprepTask*)dalloc(enc_allocs, tasks.size() * sizeof(ConvWprepTask) / sizeof(float) + 4);
            HIP_CHECK(hipMemcpy(enc_wprep[ei], tasks.data(), tasks.size() * sizeof(ConvWprepTask), hipMemcpyHostToDevice));
        }
    }

    // Fragment-major weight copies for fql_chain_kernel (needs P): BC flow with >= 3 equal hidden layers of width 256 / 512
    void build_chain_weights() {
        const Net& n = nets[NET_BC];
        const int nh = n.nl() - 1;
        const int H = n.layers[0].out_p;
        bool ok = has(K_CHAIN) && !cfg.actor_layer_norm && cfg.act_dim <= 15 && nh >= 3 && (H == 256 || H == 512);
        for (int l = 0; l < nh && ok; ++l) ok = n.layers[l].out == H && n.layers[l].out_p == H;
        use_chain = ok;
        if (!ok) return;
        const int od = cfg.obs_dim, ap = pad16(cfg.act_dim);
        std::vector<WfragTask> tasks;
        int tile = 0;
        const bool split = cfg.precision == 2;   // fql_chain_split_kernel reads pre-split bf16 hi / lo operands (same bytes)
        auto add = [&](const float* src, int K, int N, int ld, int kvalid, int split_mode) {
            float* dst = dalloc(chain_allocs, (size_t)K * N);
            tasks.push_back(WfragTask{src, dst, K, N, ld, kvalid, tile, split ? split_mode : 0});
            tile += ((K / 4) * N + FQL_THREADS - 1) / FQL_THREADS;
            return dst;
        };
        wf_bc.clear();
        for (int l = 1; l < nh; ++l) wf_bc.push_back(add(P + n.layers[l].w, H, H, H, H, 1));
        const Layer& l0 = n.layers[0];
        wf_w0 = add(P + l0.w + (size_t)od * l0.out_p, 16, H, l0.out_p, std::min(16, l0.in_p - od), 2);   // rows of (action block, t, padding)
        wf_w4 = add(P + n.layers[nh].w, H, ap, ap, H, 1);
        wfrag_n = (int)tasks.size(); wfrag_grid = tile;
        d_wfrag = (WfragTask*)dalloc(chain_allocs, tasks.size() * sizeof(WfragTask) / sizeof(float) + 4);
        HIP_CHECK(hipMemcpy(d_wfrag, tasks.data(), tasks.size() * sizeof(WfragTask), hipMemcpyHostToDevice));
        h_wfrag = tasks;
    }
    // after any out-of-graph parameter write (init, fql_set_param): bring the copies up to date
    void refresh_chain_weights(hipStream_t s) {
        if (!use_chain) return;
        hipLaunchKernelGGL(fql_wfrag_kernel, dim3(wfrag_grid), dim3(FQL_THREADS), 0, s, (const WfragTask*)d_wfrag, wfrag_n, -1);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    }

    // A trainable leaf of one segment: a vector [cols] or a matrix [rows, cols] at `off`, padded to rp x cp.  It takes the next train id
    // (n_train_leaves counts them while build_leaves runs).
    void add_leaf(const std::string& name, bool matrix, int rows, int cols, size_t off, int rp, int cp) {
        Leaf lf;
        lf.name = name;
        int d = 0;
        if (matrix) lf.shape[d++] = rows;
        lf.shape[d++] = cols;
        lf.ndim = d;
        for (int k = d; k < 4; ++k) lf.shape[k] = 1;
        lf.segs.push_back(Segment{off, matrix ? rows : 1, cols, matrix ? rp : 1, cp});
        lf.trainable = true;
        lf.train_id = n_train_leaves++;
        leaves.push_back(lf);
    }
    void build_leaves() {
        leaves.clear();
        const KindDesc& kd = desc();
        const char* bare = kd.bare;
        auto special = [&](LeafSite at, const Mod* m) { return kd.special_leaves && kd.special_leaves(*this, at, m); };
        n_train_leaves = 0;
        if (bare) {   // agents/bc.py:26-44: a bare TrainState: Dense_0 (the head), then MLP_0/Dense_i and MLP_0/LayerNorm_i (jax dict order)
            const Net& n0 = nets[NET_BC];
            auto add = [&](const std::string& name, bool matrix, int rows, int cols, size_t o0, int rp, int cp) {
                add_leaf(bare + name, matrix, rows, cols, o0, rp, cp);
            };
            const Layer& hd = n0.layers.back();
            add("Dense_0/bias", false, 1, hd.out, hd.b, 1, hd.out_p);
            add("Dense_0/kernel", true, hd.in, hd.out, hd.w, hd.in_p, hd.out_p);
            special(LS_BARE_HEAD, nullptr);
            for (int i = 0; i + 1 < n0.nl(); ++i) {
                const Layer& a = n0.layers[i];
                add("MLP_0/Dense_" + std::to_string(i) + "/bias", false, 1, a.out, a.b, 1, a.out_p);
                add("MLP_0/Dense_" + std::to_string(i) + "/kernel", true, a.in, a.out, a.w, a.in_p, a.out_p);
            }
            for (int i = 0; i + 1 < n0.nl(); ++i) {
                const Layer& a = n0.layers[i];
                if (!a.ln) continue;
                add("MLP_0/LayerNorm_" + std::to_string(i) + "/bias", false, 1, a.out, a.be, 1, a.out_p);
                add("MLP_0/LayerNorm_" + std::to_string(i) + "/scale", false, 1, a.out, a.g, 1, a.out_p);
            }
        }
        for (int mi = 0; mi < kd.nmods; ++mi) {
            const Mod& m = kd.mods[mi];
            if (m.n0 < 0) { special(LS_NO_NET, &m); continue; }
            const Net& n0 = nets[m.n0];
            const bool ens = m.n1 >= 0;
            if (visual) {
                // "<module>/encoder/..." sorts before "mlp" / "value_net"; inside: MLP_0 < stack_blocks_* (flax auto names,
                // utils/encoders.py:72-79,98); the encoder is NOT ensembled (utils/networks.py:186-187: applied before value_net)
                const EncNet& en = encs[m.enc];
                auto add_plain = [&](const std::string& name, std::vector<int64_t> shape, size_t off, int rows, int cols) {
                    Leaf lf;
                    lf.name = name;
                    lf.ndim = (int)shape.size();
                    for (int k = 0; k < 4; ++k) lf.shape[k] = k < lf.ndim ? shape[k] : 1;
                    lf.segs.push_back(Segment{off, rows, cols, rows, cols});
                    lf.trainable = m.train;
                    lf.train_id = m.train ? n_train_leaves++ : -1;
                    leaves.push_back(lf);
                };
                const std::string eb = std::string(m.name) + "/encoder/";
                add_plain(eb + "MLP_0/Dense_0/bias", {en.dense.out}, en.dense.b, 1, en.dense.out);
                add_plain(eb + "MLP_0/Dense_0/kernel", {en.dense.in, en.dense.out}, en.dense.w, en.dense.in, en.dense.out);
                for (size_t s = 0; s < en.stacks.size(); ++s)
                    for (size_t j = 0; j < en.stacks[s].conv.size(); ++j) {
                        const ConvL& c = en.stacks[s].conv[j];
                        const std::string cb = eb + "stack_blocks_" + std::to_string(s) + "/Conv_" + std::to_string(j);
                        add_plain(cb + "/bias", {c.cout}, c.b, 1, c.cout);
                        add_plain(cb + "/kernel", {3, 3, c.cin, c.cout}, c.w, 9 * c.cin, c.cout);
                    }
            }
            auto add = [&](const std::string& name, bool matrix, int rows, int cols, size_t o0, size_t o1, int rp, int cp) {
                Leaf lf;
                lf.name = name;
                int d = 0;
                if (ens) lf.shape[d++] = 2;
                if (matrix) lf.shape[d++] = rows;
                lf.shape[d++] = cols;
                lf.ndim = d;
                for (int k = d; k < 4; ++k) lf.shape[k] = 1;
                lf.segs.push_back(Segment{o0, matrix ? rows : 1, cols, matrix ? rp : 1, cp});
                if (ens) lf.segs.push_back(Segment{o1, matrix ? rows : 1, cols, matrix ? rp : 1, cp});
                lf.trainable = m.train;
                lf.train_id = m.train ? n_train_leaves++ : -1;
                leaves.push_back(lf);
            };
            const std::string base = std::string(m.name) + "/" + m.sub + "/";
            // jax dict order: Dense_0..Dense_L (bias, kernel), then LayerNorm_0.. (bias, scale); an Actor's last layer is mean_net, after actor_net
            for (int i = 0; i < (m.actor ? n0.nl() - 1 : n0.nl()); ++i) {
                const Layer& a = n0.layers[i];
                const Layer* b = ens ? &nets[m.n1].layers[i] : nullptr;
                add(base + "Dense_" + std::to_string(i) + "/bias", false, 1, a.out, a.b, b ? b->b : 0, 1, a.out_p);
                add(base + "Dense_" + std::to_string(i) + "/kernel", true, a.in, a.out, a.w, b ? b->w : 0, a.in_p, a.out_p);
            }
            for (int i = 0; i < n0.nl(); ++i) {
                const Layer& a = n0.layers[i];
                if (!a.ln) continue;
                const Layer* b = ens ? &nets[m.n1].layers[i] : nullptr;
                add(base + "LayerNorm_" + std::to_string(i) + "/bias", false, 1, a.out, a.be, b ? b->be : 0, 1, a.out_p);
                add(base + "LayerNorm_" + std::to_string(i) + "/scale", false, 1, a.out, a.g, b ? b->g : 0, 1, a.out_p);
            }
            if (m.actor && !special(LS_ACTOR_HEAD, &m)) {
                const Layer& a = n0.layers.back();
                const std::string hb = std::string(m.name) + "/mean_net/";
                add(hb + "bias", false, 1, a.out, a.b, 0, 1, a.out_p);
                add(hb + "kernel", true, a.in, a.out, a.w, 0, a.in_p, a.out_p);
            }
        }
        special(LS_LAST, nullptr);
        if (n_train_leaves > 256) invalid("too many trainable leaves (%d)", n_train_leaves);
        // Adam chunks: contiguous pieces of one leaf, <= 4096 elements
        std::vector<AdamChunk> ch;
        for (const Leaf& lf : leaves) {
            if (!lf.trainable) continue;
            for (const Segment& s : lf.segs) {
                if (s.chunk_w > 0) {   // a column block of a wider layer: one chunk per padded row
                    for (int r = 0; r < s.rows_p; ++r) ch.push_back(AdamChunk{(int)(s.off + (size_t)r * s.cols_p), s.chunk_w, lf.train_id});
                    continue;
                }
                const size_t len = (size_t)s.rows_p * s.cols_p;
                for (size_t o = 0; o < len; o += 4096)
                    ch.push_back(AdamChunk{(int)(s.off + o), (int)std::min<size_t>(4096, len - o), lf.train_id});
            }
        }
        n_chunks = (int)ch.size();
        HIP_CHECK(hipMalloc((void**)&d_chunks, ch.size() * sizeof(AdamChunk)));
        HIP_CHECK(hipMemcpy(d_chunks, ch.data(), ch.size() * sizeof(AdamChunk), hipMemcpyHostToDevice));
        std::vector<int> range(n_train_leaves + 1, 0);  // chunks are emitted leaf by leaf: contiguous ranges
        for (const AdamChunk& c : ch) range[c.leaf + 1]++;
        for (int i = 0; i < n_train_leaves; ++i) range[i + 1] += range[i];
        {   // leaves (and so chunks) are ordered module by module: actor_bc_flow, actor_onestep_flow, critic
            const char* const* mods = kd.trained;
            for (int m = 0; m < 3; ++m) {
                if (!mods[m]) { mod_chunk0[m] = 0; mod_chunkn[m] = n_chunks; continue; }
                int lo = 1 << 30, hi = -1;
                for (const Leaf& lf : leaves)
                    if (lf.trainable && lf.name.rfind(mods[m], 0) == 0) { lo = std::min(lo, lf.train_id); hi = std::max(hi, lf.train_id); }
                mod_chunk0[m] = range[lo];
                mod_chunkn[m] = range[hi + 1] - range[lo];
            }
        }
        HIP_CHECK(hipMalloc((void**)&d_leaf_range, range.size() * sizeof(int)));
        HIP_CHECK(hipMemcpy(d_leaf_range, range.data(), range.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMalloc((void**)&d_partials, (size_t)n_chunks * 4 * sizeof(float)));
        HIP_CHECK(hipMemset(d_partials, 0, (size_t)n_chunks * 4 * sizeof(float)));
        // zeroed here and never again: the workgroup that finds the launch complete puts the counter back to 0 (fql_adam_body)
        HIP_CHECK(hipMalloc((void**)&d_ticket, 16));
        HIP_CHECK(hipMemset(d_ticket, 0, 16));
    }

    const Leaf* find_leaf(const char* name) const {
        for (const Leaf& l : leaves)
            if (l.name == name) return &l;
        return nullptr;
    }
    static size_t leaf_count(const Leaf& l) {
        size_t n = 1;
        for (int i = 0; i < l.ndim; ++i) n *= (size_t)l.shape[i];
        return n;
    }
    void leaf_io(const Leaf& lf, float* arena, float* host, bool to_device) {
        HIP_CHECK(hipStreamSynchronize(stream));
        size_t ho = 0;
        for (const Segment& s : lf.segs) {
            HIP_CHECK(hipMemcpy2D(to_device ? (void*)(arena + s.off) : (void*)(host + ho), (to_device ? s.cols_p : s.cols) * sizeof(float),
                                  to_device ? (const void*)(host + ho) : (const void*)(arena + s.off),
                                  (to_device ? s.cols : s.cols_p) * sizeof(float), s.cols * sizeof(float), s.rows,
                                  to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
            ho += (size_t)s.rows * s.cols;
        }
    }

    void init_params() {
        // utils/networks.py:9-11 Glorot-uniform kernels; flax Dense bias 0; LayerNorm scale 1 / bias 0;
        // agents/fql.py:241-242 target := critic.  (Host RNG: JAX's threefry init is not reproducible.)
        const KindDesc& kd = desc();
        std::vector<float> h(n_total, 0.f);
        std::mt19937_64 gen(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull);
        for (int ni = 0; ni <= NET_OS; ++ni)
            for (const Layer& L : nets[ni].layers) {
                // an Actor's mean_net: variance_scaling(the row's scale, fan_avg, uniform) (utils/networks.py:9-11,117)
                const bool actor_head = ni == NET_BC && &L == &nets[ni].layers.back();
                const double scale = actor_head && kd.head_scale ? kd.head_scale(*this) : 1.0;
                if (actor_head && kd.head_init == HI_LECUN_TRUNC) {
                    // a bare nn.Dense (agents/bc.py:43): flax's default lecun_normal = variance_scaling(1, fan_in,
                    // truncated_normal): N(0, 1) truncated to [-2, 2], scaled by sqrt(1 / fan_in) / 0.87962566103423978
                    const double sd = std::sqrt(1.0 / (double)L.in) / 0.87962566103423978;
                    std::normal_distribution<double> Nd(0.0, 1.0);
                    for (int r = 0; r < L.in; ++r)
                        for (int c = 0; c < L.out; ++c) {
                            double v = Nd(gen);
                            while (v < -2.0 || v > 2.0) v = Nd(gen);
                            h[L.w + (size_t)r * L.out_p + c] = (float)(sd * v);
                        }
                    continue;
                }
                if (actor_head && kd.head_init == HI_TWO_HEADS) {
                    // SAC's mean_net and log_std_net: variance_scaling(actor_fc_scale, fan_avg, uniform), [H, act] each (utils/networks.py:9-11,111-113)
                    const int ad = cfg.act_dim, ap = pad16(ad);
                    const double lim = std::sqrt(6.0 * scale / (double)(L.in + ad));
                    std::uniform_real_distribution<double> U(-lim, lim);
                    for (int c0 : {0, ap})
                        for (int r = 0; r < L.in; ++r)
                            for (int c = 0; c < ad; ++c) h[L.w + (size_t)r * L.out_p + c0 + c] = (float)U(gen);
                    continue;
                }
                const double lim = std::sqrt(6.0 * scale / (double)(L.in + L.out));
                std::uniform_real_distribution<double> U(-lim, lim);
                for (int r = 0; r < L.in; ++r)
                    for (int c = 0; c < L.out; ++c) h[L.w + (size_t)r * L.out_p + c] = (float)U(gen);
                if (L.ln)
                    for (int c = 0; c < L.out; ++c) h[L.g + c] = 1.0f;
            }
        if (visual)
            for (int ei = 0; ei <= ENC_OS; ++ei) {   // xavier_uniform convolutions (utils/encoders.py:18), Glorot Dense, zero biases
                const EncNet& en = encs[ei];
                for (const EncStack& st : en.stacks)
                    for (const ConvL& c : st.conv) {
                        const double lim = std::sqrt(6.0 / (9.0 * c.cin + 9.0 * c.cout));
                        std::uniform_real_distribution<double> U(-lim, lim);
                        for (size_t i = 0; i < (size_t)9 * c.cin * c.cout; ++i) h[c.w + i] = (float)U(gen);
                    }
                const Layer& D = en.dense;
                const double lim = std::sqrt(6.0 / (double)(D.in + D.out));
                std::uniform_real_distribution<double> U(-lim, lim);
                for (size_t i = 0; i < (size_t)D.in * D.out; ++i) h[D.w + i] = (float)U(gen);
            }
        if (kd.embed_init) {   // nn.Embed's default init, variance_scaling(1.0, 'fan_in', 'normal', out_axis=0): the untruncated N(0, 1 / fan_in)
            const EmbedInit em = kd.embed_init(*this);
            std::normal_distribution<double> Nd(0.0, std::sqrt(1.0 / (double)em.fan_in));
            for (int i = 0; i < em.n; ++i) h[emb_off + i] = (float)Nd(gen);
        }
        std::memcpy(h.data() + n_train, h.data(), critic_size * sizeof(float));
        HIP_CHECK(hipMemcpy(P, h.data(), n_total * sizeof(float), hipMemcpyHostToDevice));
    }

    // ---------------------------------------------------------------------------------------
    // pass buffers
    // ---------------------------------------------------------------------------------------
    PassBuf make_pass(std::vector<void*>& owner, int net, int M, float* x0, bool bwd, bool input_grad) {
        const Net& n = nets[net];
        PassBuf p;
        p.net = net; p.M = M; p.x0 = x0;
        const int L = n.nl() - 1;
        for (int l = 0; l < L; ++l) {
            const int H = n.layers[l].out_p;
            p.g.push_back(dalloc(owner, (size_t)M * H));
            p.z.push_back(dalloc(owner, (size_t)M * H));
            if (n.layers[l].ln) {
                p.xn.push_back(dalloc(owner, (size_t)M * H));
                p.stats.push_back(dalloc(owner, (size_t)M * 2));
                p.lnpart.push_back(dalloc(owner, (size_t)M * ((2 * ((H + 31) / 32) + 3) & ~3)));   // (sum, sum sq) per 32 columns
            } else {
                p.xn.push_back(p.g.back());
                p.stats.push_back(nullptr);
                p.lnpart.push_back(nullptr);
            }
        }
        p.out = dalloc(owner, (size_t)M * n.layers[L].out_p);
        if (bwd) {
            for (int l = 0; l <= L; ++l) p.dz.push_back(dalloc(owner, (size_t)M * n.layers[l].out_p));
            for (int l = 0; l < L; ++l) p.dy.push_back(n.layers[l].ln ? dalloc(owner, (size_t)M * n.layers[l].out_p) : nullptr);
            if (input_grad) p.dx0 = dalloc(owner, (size_t)M * n.in_p());
        }
        return p;
    }

    // ---------------------------------------------------------------------------------------
    // visual path: encoder passes (utils/encoders.py:61-100) as conv / pool / GEMM ops of the same program
    // ---------------------------------------------------------------------------------------
    EncBuf make_enc_buf(std::vector<void*>& owner, int enc, int n, const unsigned char* img, bool bwd) {
        const EncNet& en = encs[enc];
        EncBuf b;
        b.enc = enc; b.n = n; b.img = img;
        auto al = [&](size_t nfloats) {
            float* p = dalloc(owner, nfloats);
            b.bytes[p] = std::max<size_t>(nfloats, 4) * sizeof(float);
            return p;
        };
        size_t maxel = 0;
        for (const EncStack& st : en.stacks) {
            EncBuf::St s;
            const int C = st.conv[0].cout;
            const size_t full = (size_t)n * st.H * st.W * C, quarter = full / 4;
            maxel = std::max(maxel, full);
            s.c0 = al(full);
            s.pool = al(quarter);
            s.arg = (unsigned char*)al(quarter / 4 + 4);
            for (size_t j = 1; j + 1 < st.conv.size(); j += 2) {
                s.c1.push_back(al(quarter));
                s.y.push_back(al(quarter));
            }
            b.st.push_back(s);
        }
        b.frelu = al((size_t)n * en.flat);
        b.z = al((size_t)n * enc_dim);
        b.E = al((size_t)n * enc_dim);
        if (bwd) {
            b.dz = al((size_t)n * enc_dim);
            b.dA = al(maxel); b.dB = al(maxel); b.dC = al(maxel);
            for (const EncStack& st : en.stacks)
                for (const ConvL& c : st.conv) b.wpart[P + c.w] = dalloc(owner, (size_t)256 * (9 * pad16c(c.cin) + 1) * c.cout);
        }
        return b;
    }
    // image rows per workgroup: <= 8 MFMA row tiles of 16 pixels, whole rows, LDS within 64 KB
    // The halving sequence from the cap is the planner's choice wherever it finds a fit (every tiling it picks stays as it is); only when it
    // finds none (12-pixel rows: 10, 5, 2, 1 never try 8 or 4) the largest fitting R below the cap is taken.  The weight gradient of a float
    // input stages its (R + 2) halo rows through ConvTile's NF float4 per thread: a tile beyond that would leave LDS rows unwritten.
    static int conv_rows(int H, int W, int Ci, int Co, bool wgrad, bool u8 = false) {
        const int cap = std::min(H, std::max(1, 128 / W));
        auto fits = [&](int R) {
            if (H % R || (R * W) % 16) return false;
            if (wgrad && !u8 && (R + 2) * (W + 2) * (Ci / 4) > ConvTile::NF * FQL_THREADS) return false;
            const size_t fl = wgrad ? (size_t)(R + 2) * (W + 2) * (Ci + 4) + (size_t)R * W * (Co + 4)
                                    : (size_t)(R + 2) * (W + 2) * (Ci + 4) + (size_t)Co * (9 * Ci + 4);
            return fl * sizeof(float) <= 65536;
        };
        for (int R = cap; R >= 1; R >>= 1)
            if (fits(R)) return R;
        for (int R = cap; R >= 1; --R)
            if (fits(R)) return R;
        invalid("convolution tile does not fit (H %d, W %d, channels %d -> %d)", H, W, Ci, Co);
    }
    void emit_conv(Program& pr, const void* in, const void* in_id, int in_mode, int n, int H, int W, const ConvL& c, bool transposed,
                   float* out, const void* out_id, float* out_relu, const float* mask, const void* mask_id, const float* add, const void* add_id) {
        Op op{};
        op.type = in_mode == 2 ? OP_CONV_U8 : OP_CONV;
        if (in_mode == 2 && (transposed || c.cout != 16)) invalid("uint8 convolution kernel: 16 output channels expected (got %d)", c.cout);
        ConvArgs& a = op.conv;
        a.in = in; a.Wl = transposed ? c.Wb : c.Wf; a.bias = transposed ? nullptr : P + c.b;
        a.out = out; a.out_relu = out_relu; a.mask = mask; a.add = add;
        a.N = n; a.H = H; a.W = W;
        if (!transposed) { a.Ci = pad16c(c.cin); a.Ci_real = c.cin; a.Co = c.cout; }
        else { a.Ci = c.cout; a.Ci_real = c.cout; a.Co = c.cin; }
        a.in_mode = in_mode; a.transposed = transposed ? 1 : 0;
        a.R = conv_rows(H, W, a.Ci, a.Co, false);
        op.reads = {in_id, a.Wl};
        if (!transposed) op.reads.push_back(P + c.b);
        if (mask) op.reads.push_back(mask_id);
        if (add) op.reads.push_back(add_id);
        op.writes = {out_id};
        if (out_relu) op.writes.push_back(out_relu);
        push(pr, op);
    }
    void emit_encoder_forward(Program& pr, EncBuf& b) {
        const EncNet& en = encs[b.enc];
        const int n = b.n;
        {   // this pass's weights in LDS layout (forward and data-gradient forms), one small launch per encoder pass
            Op op{};
            op.type = OP_CONV_WPREP;
            op.wprep_tasks = enc_wprep[b.enc];   // (the payload: the passes of one level merge into one launch; alone, this one)
            op.wprep_n = enc_nconv[b.enc];
            op.k = bind_wprep(op.wprep_tasks, op.wprep_n);
            for (const EncStack& st : en.stacks)
                for (const ConvL& c : st.conv) {
                    op.reads.push_back(P + c.w);
                    op.writes.push_back(c.Wf);
                    if (c.Wb) op.writes.push_back(c.Wb);
                }
            push(pr, op);
        }
        const float* x = nullptr;
        for (size_t s = 0; s < en.stacks.size(); ++s) {
            const EncStack& st = en.stacks[s];
            EncBuf::St& bs = b.st[s];
            const int C = st.conv[0].cout, H2 = st.H / 2, W2 = st.W / 2;
            // a stack's first convolution and its max-pool as one kernel: the pre-pool tensor (for stack 0 the largest write of the update) is never materialised
            const bool fuse_pool = st.conv[0].pool_fused;
            if (s == 0) emit_conv(pr, b.img, b.img, 2, n, st.H, st.W, st.conv[0], false, bs.c0, bs.c0, nullptr, nullptr, nullptr, nullptr, nullptr);
            else emit_conv(pr, x, x, 0, n, st.H, st.W, st.conv[0], false, bs.c0, bs.c0, nullptr, nullptr, nullptr, nullptr, nullptr);
            if (fuse_pool) {
                Op& co = pr.ops.back();
                co.conv.out = bs.pool; co.conv.parg = bs.arg;
                co.writes = {bs.pool, bs.arg};
            } else
            {
                const PoolArgs a{bs.c0, bs.pool, bs.arg, n, st.H, st.W, C};
                const size_t tot = (size_t)a.N * (a.H / 2) * (a.W / 2) * (a.C / 4);
                emit(pr, OP_POOL, bind(fql_maxpool_kernel, (tot + FQL_THREADS - 1) / FQL_THREADS, a), {bs.c0}, {bs.pool, bs.arg});
            }
            const float* y = bs.pool;
            for (size_t blk = 0; blk < bs.c1.size(); ++blk) {
                const bool last = s + 1 == en.stacks.size() && blk + 1 == bs.c1.size();
                emit_conv(pr, y, y, 1, n, H2, W2, st.conv[1 + 2 * blk], false, bs.c1[blk], bs.c1[blk], nullptr, nullptr, nullptr, nullptr, nullptr);
                emit_conv(pr, bs.c1[blk], bs.c1[blk], 1, n, H2, W2, st.conv[2 + 2 * blk], false, bs.y[blk], bs.y[blk], last ? b.frelu : nullptr,
                          nullptr, nullptr, y, y);
                y = bs.y[blk];
            }
            x = y;
        }
        Op op{};   // MLP((512,), activate_final=True): Dense + GELU (utils/encoders.py:98)
        op.type = OP_GEMM;
        GemmTask& t = op.gemm;
        const Layer& D = en.dense;
        t.A = b.frelu; t.lda = D.in_p;
        t.B = P + D.w; t.ldb = D.out_p; t.bias = P + D.b;
        t.C = b.E; t.ldc = D.out_p; t.Zout = b.z;
        t.M = n; t.N = D.out_p; t.K = D.in_p;
        t.flags = GF_BIAS | GF_GELU | GF_SAVE_Z;
        op.reads = {t.A, t.B};
        op.writes = {t.C, t.Zout};
        // (the LDS-tiled kernel whichever lane this pass is on: K = flat does not fit the 16-row kernel's A tile)
        if (t.M % 64 == 0 && t.N % 64 == 0 && t.K % 64 == 0) op.type = OP_GEMM64;
        else if (t.K > 1024) invalid("encoder Dense with %d inputs needs a batch that is a multiple of 64", t.K);
        push(pr, op);
    }
    void emit_conv_wgrad(Program& pr, EncBuf& b, const void* in, const void* in_id, int in_mode, int n, int H, int W, const ConvL& c,
                         const float* dout, const void* dout_id) {
        Op op{};
        op.type = OP_CONV_WGRAD;
        ConvWgradArgs& a = op.cw;
        float* wp = b.wpart.at(P + c.w);
        a.in = in; a.dout = dout; a.partial = wp;
        a.N = n; a.H = H; a.W = W; a.Ci = pad16c(c.cin); a.Ci_real = c.cin; a.Co = c.cout; a.in_mode = in_mode;
        if (in_mode == 2 && (a.Ci != 16 || a.Co != 16)) invalid("uint8 convolution weight gradient: <= 16 input channels and 16 output channels expected (got %d -> %d)", c.cin, c.cout);
        a.R = conv_rows(H, W, a.Ci, a.Co, true, in_mode == 2);
        a.nblocks = n * (H / a.R);
        constexpr int cwg_grid = 256;   // persistent workgroups per weight-gradient task
        op.cw_grid = std::min(a.nblocks, cwg_grid);
        op.reads = {in_id, dout_id};
        op.writes = {wp};
        push(pr, op);
        Op r{};
        r.type = OP_CONV_WRED;
        r.cwr = ConvWredArgs{wp, G + c.w, G + c.b, op.cw_grid, a.Ci, a.Co, c.cin, 0};
        r.reads = {wp};
        r.writes = {G + c.w, G + c.b};
        push(pr, r);
    }
    // backward of images [img0, img0 + n) of pass b; the encoding's gradient = first enc_dim columns of dxa (+ dxb)
    void emit_encoder_backward(Program& pr, EncBuf& b, int img0, int n, const float* dxa, const float* dxb, int ld, const void* align_with = nullptr) {
        const EncNet& en = encs[b.enc];
        const Layer& D = en.dense;
        {
            const EncDzArgs a{dxa, dxb, b.z + (size_t)img0 * enc_dim, b.dz, n, enc_dim, ld};
            Op& op = emit(pr, OP_ENC_DZ, bind(fql_enc_dz_kernel, (a.M * a.n + FQL_THREADS - 1) / FQL_THREADS, a), {dxa, b.z}, {b.dz});
            if (dxb) op.reads.push_back(dxb);
            // level alignment: the three encoder backward passes start together so that their per-level convolutions,
            // weight gradients and partial folds share launches (the lane is serial either way)
            if (align_with) op.reads.push_back(align_with);
        }
        {
            Op op{};
            op.type = OP_WGRAD;
            WgradTask& w = op.wgrad;
            w.X = b.frelu + (size_t)img0 * en.flat; w.ldx = D.in_p;
            w.dZ = b.dz; w.ldz = D.out_p;
            w.dW = G + D.w; w.ldw = D.out_p; w.db = G + D.b;
            w.M = n; w.Kin = D.in_p; w.N = D.out_p;
            op.reads = {b.frelu, b.dz};
            op.writes = {w.dW, w.db};
            push(pr, op);
        }
        const EncStack& lst = en.stacks.back();
        const float* xfinal = b.st.back().y.empty() ? b.st.back().pool : b.st.back().y.back();
        {
            Op op{};   // d(flat) = dz W^T, through the final ReLU (utils/encoders.py:92)
            op.type = OP_GEMM;
            GemmTask& t = op.gemm;
            t.A = b.dz; t.lda = D.out_p;
            t.B = P + D.w; t.ldb = D.out_p;
            t.C = b.dA; t.ldc = D.in_p;
            t.M = n; t.N = D.in_p; t.K = D.out_p;
            t.flags = GF_TRANS_B | GF_RELUGRAD;
            t.Zprev = xfinal + (size_t)img0 * en.flat;
            op.reads = {b.dz, t.B, xfinal};
            op.writes = {b.dA};
            if (t.M % 64 == 0 && t.N % 64 == 0 && t.K % 64 == 0) op.type = OP_GEMM64;
            push(pr, op);
        }
        (void)lst;
        float* dy = b.dA;
        std::vector<float*> freeb = {b.dB, b.dC};
        auto take = [&]() { float* p = freeb.back(); freeb.pop_back(); return p; };
        for (int s = (int)en.stacks.size() - 1; s >= 0; --s) {
            const EncStack& st = en.stacks[s];
            EncBuf::St& bs = b.st[s];
            const int C = st.conv[0].cout, H2 = st.H / 2, W2 = st.W / 2;
            const size_t q_img = (size_t)H2 * W2 * C, f_img = (size_t)st.H * st.W * C;
            for (int blk = (int)bs.c1.size() - 1; blk >= 0; --blk) {
                const float* inp = blk == 0 ? bs.pool : bs.y[blk - 1];
                const float* c1 = bs.c1[blk];
                const float* inp_o = inp + (size_t)img0 * q_img;
                const float* c1_o = c1 + (size_t)img0 * q_img;
                emit_conv_wgrad(pr, b, c1_o, c1, 1, n, H2, W2, st.conv[2 + 2 * blk], dy, dy);
                float* d_c1 = take();
                emit_conv(pr, dy, dy, 0, n, H2, W2, st.conv[2 + 2 * blk], true, d_c1, d_c1, nullptr, c1_o, c1, nullptr, nullptr);
                emit_conv_wgrad(pr, b, inp_o, inp, 1, n, H2, W2, st.conv[1 + 2 * blk], d_c1, d_c1);
                float* dy_new = take();
                emit_conv(pr, d_c1, d_c1, 0, n, H2, W2, st.conv[1 + 2 * blk], true, dy_new, dy_new, nullptr, inp_o, inp, dy, dy);
                freeb.push_back(d_c1); freeb.push_back(dy);
                dy = dy_new;
            }
            float* d_c0 = take();
            {
                const PoolBwdArgs a{dy, bs.arg + (size_t)img0 * q_img, d_c0, n, st.H, st.W, C};
                const size_t tot = (size_t)a.N * a.H * a.W * (a.C / 4);
                emit(pr, OP_POOL_BWD, bind(fql_maxpool_bwd_kernel, (tot + FQL_THREADS - 1) / FQL_THREADS, a), {dy, bs.arg}, {d_c0});
            }
            if (s == 0) {
                const size_t ib = (size_t)st.H * st.W * st.conv[0].cin;
                emit_conv_wgrad(pr, b, b.img + (size_t)img0 * ib, b.img, 2, n, st.H, st.W, st.conv[0], d_c0, d_c0);
            } else {
                const EncBuf::St& ps = b.st[s - 1];
                const float* xin = ps.y.empty() ? ps.pool : ps.y.back();
                const size_t xi = (size_t)st.H * st.W * st.conv[0].cin;
                emit_conv_wgrad(pr, b, xin + (size_t)img0 * xi, xin, 0, n, st.H, st.W, st.conv[0], d_c0, d_c0);
                float* dprev = take();
                emit_conv(pr, d_c0, d_c0, 0, n, st.H, st.W, st.conv[0], true, dprev, dprev, nullptr, nullptr, nullptr, nullptr, nullptr);
                freeb.push_back(dy);
                dy = dprev;
            }
            freeb.push_back(d_c0);
            (void)f_img;
        }
    }

    // throughput-lane tasks with 64-aligned shapes go to the 64x64 LDS-tiled kernel
    bool want64(int M, int N, int K, int flags) const {
        if ((emit_lane == 0 && !lane0_64) || !allow64) return false;
        if (M % 64 || N % 64 || K % 64) return false;
        if (flags & (GF_EULER | GF_CLIP_OUT)) return false;
        return true;
    }

    // per-pass placement: lane and kernel family (FQL_LANE_<pass> overrides the lane: tests/test_gpu_streams.py provokes the refusal of a two-way edge with it)
    void place(const char* pass, int default_lane, bool default64) {
        char key[64];
        snprintf(key, sizeof key, "FQL_LANE_%s", pass);
        const char* e = getenv(key);
        emit_lane = e ? atoi(e) : default_lane;
        allow64 = default64;
    }

    void push(Program& pr, Op& op) {
        op.lane = emit_lane;
        pr.ops.push_back(op);
    }
    // a single-op launch appended on emit_lane: the bound launch and the buffers it reads and writes.  The reference is for the sites that
    // append conditional reads or writes (it holds until the next op is pushed).
    Op& emit(Program& pr, OpType type, const Bound& k, std::vector<const void*> reads, std::vector<const void*> writes) {
        Op op{};
        op.type = type;
        op.k = k;
        op.reads = std::move(reads);
        op.writes = std::move(writes);
        push(pr, op);
        return pr.ops.back();
    }

    // forward of one pass appended to a program.  final_flags: epilogue of the last layer.
    // first_layer > 0: the layers before it were run by the caller (BC's sampler builds layer 0's output itself).
    void emit_forward(Program& pr, const PassBuf& p, bool save, int final_flags = 0, float* aux = nullptr,
                      float* aux2 = nullptr, float f0 = 0.f, float f1 = 0.f, int first_layer = 0) {
        const Net& n = nets[p.net];
        const int L = n.nl() - 1;
        for (int l = first_layer; l <= L; ++l) {
            const Layer& ly = n.layers[l];
            Op op{};
            op.type = OP_GEMM;
            GemmTask& t = op.gemm;
            const bool a_ln = l > 0 && n.layers[l - 1].ln;
            t.A = (l == 0) ? p.x0 : p.g[l - 1];
            t.lda = ly.in_p;
            t.B = P + ly.w; t.ldb = ly.out_p;
            t.bias = P + ly.b;
            t.M = p.M; t.N = ly.out_p; t.K = ly.in_p;
            t.ldc = ly.out_p;
            t.flags = GF_BIAS;
            op.reads = {t.A, t.B};
            if (a_ln) {
                t.flags |= GF_A_LN;
                t.ln_g = P + n.layers[l - 1].g; t.ln_b = P + n.layers[l - 1].be;
                t.ln_width = n.layers[l - 1].out;
                if (save) {
                    t.flags |= GF_LN_WRITE;
                    t.ln_xout = p.xn[l - 1]; t.ln_stats = p.stats[l - 1];
                    op.writes.push_back(t.ln_xout);
                    op.writes.push_back(t.ln_stats);
                }
            }
            if (l < L) {
                t.C = p.g[l];
                t.flags |= GF_GELU;
                if (save) { t.flags |= GF_SAVE_Z; t.Zout = p.z[l]; op.writes.push_back(t.Zout); }
                op.writes.push_back(t.C);
                // LDS-tiled kernel; a LayerNorm'd A operand needs the producing layer's partial sums, i.e. that layer on it too
                const bool prev64 = l > 0 && want64(p.M, n.layers[l - 1].out_p, n.layers[l - 1].in_p, GF_BIAS | GF_GELU);
                if (want64(t.M, t.N, t.K, t.flags) && (!a_ln || prev64)) {
                    op.type = OP_GEMM64;
                    if (a_ln) { t.aux2 = p.lnpart[l - 1]; t.i0 = t.K / 32; op.reads.push_back(t.aux2); }
                    if (ly.ln) { t.flags |= GF_LN_PART; t.aux = p.lnpart[l]; t.i1 = t.N / 32; op.writes.push_back(t.aux); }
                }
            } else {
                t.C = p.out;
                t.flags |= final_flags;
                if (final_flags & GF_EULER) {
                    t.aux = aux; t.aux2 = aux2;
                    t.i0 = n.in_p(); t.i1 = cfg.obs_dim; t.i2 = cfg.act_dim;
                    t.f0 = f0; t.f1 = f1;
                    op.reads.push_back(aux);
                    op.writes.push_back(aux);
                    if (aux2) op.writes.push_back(aux2);
                } else {
                    op.writes.push_back(t.C);
                    if (final_flags & GF_OS_SCATTER) {
                        t.aux = aux; t.aux2 = aux2;
                        t.i0 = nets[NET_C0].in_p(); t.i1 = cfg.obs_dim; t.i2 = cfg.act_dim;
                        op.writes.push_back(aux);
                        op.writes.push_back(aux2);
                    }
                }
            }
            push(pr, op);
        }
    }

    // Euler chain with 3 launches per step instead of 5 (agents/fql.py:155-171): [fold head partials -> a_s; layer 0 as a
    // rank-(act+1) update of the loop-invariant C0 = obs W0 + b0; layer 1] , [middle layers] , [last hidden layer +
    // head partials].  The head's reduction over hidden columns crosses workgroups, so each column tile publishes its
    // 16 x ap partial and the consumer folds them in fixed order (deterministic).
    void emit_euler_fused(Program& pr) {
        const Net& n = nets[NET_BC];
        const int nh = n.nl() - 1, fs = cfg.flow_steps;
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad), inp_b = n.in_p();
        const Layer& l0 = n.layers[0];
        {
            Op op{};
            op.type = OP_GEMM;
            GemmTask& t = op.gemm;
            t.A = X_e0; t.lda = l0.in_p; t.B = P + l0.w; t.ldb = l0.out_p; t.bias = P + l0.b; t.C = C0; t.ldc = l0.out_p;
            t.M = B; t.N = l0.out_p; t.K = l0.in_p; t.flags = GF_BIAS;
            op.reads = {X_e0, t.B};
            op.writes = {C0};
            push(pr, op);
        }
        for (int s = 0; s < fs; ++s) {
            for (int l = 1; l < nh; ++l) {
                const Layer& ly = n.layers[l];
                Op op{};
                op.type = OP_GEMM;
                GemmTask& t = op.gemm;
                t.B = P + ly.w; t.ldb = ly.out_p; t.bias = P + ly.b;
                t.M = B; t.N = ly.out_p; t.K = ly.in_p; t.ldc = ly.out_p;
                t.flags = GF_BIAS | GF_GELU;
                t.i1 = ap; t.i2 = ad; t.f0 = 1.0f / (float)fs; t.f1 = (float)s / (float)fs;
                if (l == 1) {
                    t.flags |= GF_A_EULER0;
                    t.A = C0; t.lda = l0.out_p;
                    t.ew = P + l0.w + (size_t)od * l0.out_p;
                    if (s <= 1) { t.ea_in = X_eu + od; t.i0 = inp_b; } else { t.ea_in = Abuf[(s - 1) & 1]; t.i0 = ap; }
                    op.reads = {C0, t.B, (s <= 1) ? (const void*)X_eu : (const void*)Abuf[(s - 1) & 1]};
                    if (s >= 1) {
                        t.evp = Vpart; t.eb = P + n.layers[nh].b; t.e_ntp = vp_tiles; t.ea_out = Abuf[s & 1];
                        op.reads.push_back(Vpart);
                        op.reads.push_back(P + n.layers[nh].w);
                        op.writes.push_back(Abuf[s & 1]);
                    }
                } else {
                    t.A = p_eu.g[l - 1]; t.lda = ly.in_p;
                    op.reads = {t.A, t.B};
                }
                if (l == nh - 1) {  // nh >= 3: never the same task as part 1
                    t.flags |= GF_HEAD_PART;
                    t.ew4 = P + n.layers[nh].w;
                    t.evp = Vpart;
                    t.C = nullptr;
                    op.writes.push_back(Vpart);
                } else {
                    t.C = p_eu.g[l];
                    op.writes.push_back(t.C);
                }
                push(pr, op);
            }
        }
        emit_euler_finish(pr);
    }

    // the last Euler step of both fused chains: target = clip(a + (folded head partials + bias) / flow_steps)
    void emit_euler_finish(Program& pr) {
        const Net& n = nets[NET_BC];
        const int nh = n.nl() - 1, fs = cfg.flow_steps, od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        const bool from_x = fs == 1;
        const EulerFinishArgs ef{from_x ? X_eu + od : Abuf[(fs - 1) & 1], Vpart, P + n.layers[nh].b, tgt, B, ad, ap, vp_tiles,
                                 from_x ? n.in_p() : ap, 1.0f / (float)fs};
        emit(pr, OP_EULER_FIN, bind(fql_euler_finish_kernel, (ef.M * ef.ad + FQL_THREADS - 1) / FQL_THREADS, ef),
             {from_x ? (const void*)X_eu : (const void*)Abuf[(fs - 1) & 1], Vpart, P + n.layers[nh].w},   // (head bias: WAR against Adam)
             {tgt});
    }

    // XCD-aware tile order of a chain launch over M rows of an H-wide layer (16-row tiles x 32-column tiles): the number of row groups gm
    // (gm x gn = 8 blocks of the tile grid) with the fewest panel fetches, 0 = row-major when no grouping divides the grid
    static int chain_xg(int M, int H) {
        const int ntm = M / 16, ntn = H / 32;
        int xg = 0;
        double best = 1e30;
        for (int gm : {1, 2, 4, 8}) {
            const int gn = 8 / gm;
            if (ntm % gm || ntn % gn) continue;
            const double cost = (double)gn * M + (double)gm * H;
            if (cost < best) { best = cost; xg = gm; }
        }
        return xg;
    }
    // One launch of the chain kernel (fql_chain.h) over `a` (variant 0 .. 2: a link of the Euler chain; 3: a hidden layer's data gradient):
    // the instantiation for this hidden width and variant, split-bf16 operands at precision = 2 except in variant 3 (its dZ / W arrive as
    // fp32 and splitting both in the kernel costs what the MFMAs save).  The caller sets the op's reads and writes.
    Op chain_op(ChainArgs a) {
        const int H = cfg.actor_hidden[0];
        a.tl = -1;
        a.xg = chain_xg(a.M, H);
        const bool split = cfg.precision == 2 && a.variant != 3;
        const Geo g512(dim3((a.M / 16) * (512 / 32)), dim3(FQL_CHAIN_THREADS), FQL_CHAIN_LDS_BYTES(512));
        const Geo g256(dim3((a.M / 16) * (256 / 32)), dim3(FQL_CHAIN_THREADS), FQL_CHAIN_LDS_BYTES(256));
        Op op{};
        op.type = OP_CHAIN;
#define FQL_CHAIN_PICK(KERNEL, VV) (H == 512 ? bind(KERNEL<512, VV>, g512, a) : bind(KERNEL<256, VV>, g256, a))
        if (split) op.k = a.variant == 0 ? FQL_CHAIN_PICK(fql_chain_split_kernel, 0) : a.variant == 1 ? FQL_CHAIN_PICK(fql_chain_split_kernel, 1)
                                                                                                       : FQL_CHAIN_PICK(fql_chain_split_kernel, 2);
        else op.k = a.variant == 0 ? FQL_CHAIN_PICK(fql_chain_kernel, 0) : a.variant == 1 ? FQL_CHAIN_PICK(fql_chain_kernel, 1)
                  : a.variant == 2 ? FQL_CHAIN_PICK(fql_chain_kernel, 2) : FQL_CHAIN_PICK(fql_chain_kernel, 3);
#undef FQL_CHAIN_PICK
        op.k = tl_in(op.k, offsetof(ChainArgs, tl));
        op.macs = (double)a.M * H * H + (a.variant == 0 ? (double)a.M * 16.0 * H : 0.0) + (a.variant == 2 ? (double)a.M * H * a.ap : 0.0);
        return op;
    }

    // The same 3-launches-per-step chain on fql_chain_kernel (512-thread workgroups, fragment-major weights, kernarg tasks)
    bool euler_finish_fused = false;   // set per program build: the head dgrad's prologue finishes the target (GF_A_EULFIN), no OP_EULER_FIN launch
    void emit_euler_chain(Program& pr) {
        const Net& n = nets[NET_BC];
        const int nh = n.nl() - 1, fs = cfg.flow_steps;
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad), inp_b = n.in_p();
        const Layer& l0 = n.layers[0];
        {
            Op op{};
            op.type = OP_GEMM;
            GemmTask& t = op.gemm;
            t.A = X_e0; t.lda = l0.in_p; t.B = P + l0.w; t.ldb = l0.out_p; t.bias = P + l0.b; t.C = C0; t.ldc = l0.out_p;
            t.M = B; t.N = l0.out_p; t.K = l0.in_p; t.flags = GF_BIAS | (cfg.precision == 2 ? GF_C_FRAGT : GF_C_FRAG);   // the split chain runs layer 0 transposed: C0 in the transposed-tile layout
            op.reads = {X_e0, t.B};
            op.writes = {C0};
            push(pr, op);
        }
        for (int s = 0; s < fs; ++s) {
            for (int l = 1; l < nh; ++l) {
                const Layer& ly = n.layers[l];
                ChainArgs a{};
                std::vector<const void*> reads, writes;
                a.Wf = wf_bc[l - 1]; a.bias = P + ly.b;
                a.M = B; a.ad = ad; a.ap = ap;
                a.inv_steps = 1.0f / (float)fs; a.t_s = (float)s / (float)fs;
                a.variant = 1;
                reads = {a.Wf, P + ly.w};
                if (l == 1) {
                    a.variant = 0;
                    a.A = C0; a.W0f = wf_w0;
                    if (s <= 1) { a.ea_in = X_eu + od; a.ea_ld = inp_b; } else { a.ea_in = Abuf[(s - 1) & 1]; a.ea_ld = ap; }
                    reads.push_back(C0);
                    reads.push_back(wf_w0);
                    reads.push_back((s <= 1) ? (const void*)X_eu : (const void*)Abuf[(s - 1) & 1]);
                    if (s >= 1) {
                        a.evp_in = Vpart; a.eb = P + n.layers[nh].b; a.ea_out = Abuf[s & 1];
                        reads.push_back(Vpart);
                        reads.push_back(P + n.layers[nh].w);
                        writes.push_back(Abuf[s & 1]);
                    }
                } else {
                    a.A = p_eu.g[l - 1];
                    reads.push_back(a.A);
                }
                if (l == nh - 1) {   // nh >= 3: never the same launch as variant A
                    a.variant = 2;
                    a.W4f = wf_w4; a.evp_out = Vpart;
                    reads.push_back(wf_w4);
                    writes.push_back(Vpart);
                } else {
                    a.C = p_eu.g[l];
                    writes.push_back(a.C);
                }
                Op op = chain_op(a);
                op.reads = reads; op.writes = writes;
                push(pr, op);
            }
        }
        if (euler_finish_fused) return;
        emit_euler_finish(pr);
    }
    // refresh of the fragment-major copies inside a program, behind the Adam launch that rewrites the BC flow's kernels
    void emit_wfrag(Program& pr) {
        if (!use_chain) return;
        const Net& n = nets[NET_BC];
        Op op{};
        op.type = OP_WFRAG;
        op.k = tl_last(bind(fql_wfrag_kernel, wfrag_grid, d_wfrag, wfrag_n, -1));
        for (const Layer& L : n.layers) op.reads.push_back(P + L.w);
        for (float* w : wf_bc) op.writes.push_back(w);
        op.writes.push_back(wf_w0);
        op.writes.push_back(wf_w4);
        push(pr, op);
    }

    // backward of one pass: dz[L] must already hold dLoss/dOut.  rows: view [row_off, row_off+M) of a
    // taller forward pass (one-step actor: only the (obs, z) block is differentiated).
    void emit_backward(Program& pr, const PassBuf& p, int row_off, int M, bool param_grads, bool input_grad,
                       const void* align_with = nullptr) {
        size_t first_op = pr.ops.size();
        const Net& n = nets[p.net];
        const int L = n.nl() - 1;
        auto rows = [&](float* base, int ld) { return base + (size_t)row_off * ld; };
        // backward of the LayerNorm in front of layer l: dZ[l - 1] from the gradient it first reads, which the caller names in the task as dY
        // (the dgrad's output) or as dq and wq (a scalar head: dY is synthesised)
        auto ln_bwd = [&](int l, const void* first_read) {
            const Layer& prev = n.layers[l - 1];
            Op lo{};
            lo.type = OP_LNBWD;
            LnBwdTask& q = lo.ln;
            q.Z = rows(p.z[l - 1], prev.out_p);
            q.Gv = rows(p.g[l - 1], prev.out_p);
            q.stats = p.stats[l - 1] + (size_t)row_off * 2;
            q.gamma = P + prev.g;
            q.dZ = p.dz[l - 1];
            q.dgamma = param_grads ? G + prev.g : nullptr;
            q.dbeta = param_grads ? G + prev.be : nullptr;
            q.M = M; q.H = prev.out_p; q.ld = prev.out_p; q.width = prev.out;
            lo.reads = {first_read, p.z[l - 1], p.g[l - 1], p.stats[l - 1], q.gamma};
            lo.writes = {q.dZ};
            if (param_grads) { lo.writes.push_back(q.dgamma); lo.writes.push_back(q.dbeta); }
            return lo;
        };
        for (int l = L; l >= 0; --l) {
            const Layer& ly = n.layers[l];
            float* dz = p.dz[l];
            const float* xin = (l == 0) ? rows(p.x0, ly.in_p) : rows(p.xn[l - 1], ly.in_p);
            const void* xin_id = (l == 0) ? (const void*)p.x0 : (const void*)p.xn[l - 1];
            if (param_grads) {
                Op op{};
                op.type = OP_WGRAD;
                WgradTask& w = op.wgrad;
                w.X = xin; w.ldx = ly.in_p;
                w.dZ = dz; w.ldz = ly.out_p;
                w.dW = G + ly.w; w.ldw = ly.out_p;
                w.db = G + ly.b;
                w.M = M; w.Kin = ly.in_p; w.N = ly.out_p;
                op.reads = {xin_id, dz};
                op.writes = {w.dW, w.db};
                // weight gradients feed nothing but the optimizer: those of a chain that runs on the critical lane are
                // issued on the side lane so they never sit between two links of that chain (a separate wgrad lane was measured
                // slower than sharing launches)
                const int keep = emit_lane;
                if (emit_lane == 0 && !split_build && !lane0_64) emit_lane = 1;
                if (defer_wgrads) { op.lane = emit_lane; defer_wgrads->push_back(op); }
                else push(pr, op);
                emit_lane = keep;
            }
            if (l == 0 && !input_grad) break;
            if (l == L && l > 0 && ly.out == 1 && n.layers[l - 1].ln) {
                // scalar head behind a LayerNorm (critic Q): dY = dq (x) w is rank 1, synthesised inside the LN-backward
                Op lo = ln_bwd(l, dz);
                LnBwdTask& q = lo.ln;
                q.dq = dz; q.ldq = ly.out_p; q.wq = P + ly.w; q.ldw = ly.out_p;
                push(pr, lo);
                continue;
            }
            // dgrad: dX = dZ W^T
            Op op{};
            op.type = OP_GEMM;
            GemmTask& t = op.gemm;
            t.A = dz; t.lda = ly.out_p;
            t.B = P + ly.w; t.ldb = ly.out_p;
            t.M = M; t.N = ly.in_p; t.K = ly.out_p;
            t.ldc = ly.in_p;
            t.flags = GF_TRANS_B;
            op.reads = {dz, t.B};
            if (l == 0) {
                t.C = p.dx0;
                op.writes = {t.C};
                // state agents read nothing of dX0 but the action block (dQ/da; no encoder behind the observations): the lean 16-column launch
                if (!visual && cfg.precision != 1 && t.K % 512 == 0 && t.M % 16 == 0 && cfg.obs_dim + 16 <= t.N && cfg.act_dim <= 16) {
                    op.type = OP_DGRAD0;
                    t.i1 = cfg.obs_dim;
                }
                push(pr, op);
                break;
            }
            const Layer& prev = n.layers[l - 1];
            if (prev.ln) {
                t.C = p.dy[l - 1];
                op.writes = {t.C};
                if (want64(t.M, t.N, t.K, t.flags)) op.type = OP_GEMM64;
                push(pr, op);
                Op lo = ln_bwd(l, p.dy[l - 1]);
                lo.ln.dY = p.dy[l - 1];
                push(pr, lo);
            } else {
                t.C = p.dz[l - 1];
                t.flags |= GF_GELUGRAD;
                t.Zprev = rows(p.z[l - 1], prev.out_p);
                op.reads.push_back(p.z[l - 1]);
                op.writes = {t.C};
                if (want64(t.M, t.N, t.K, t.flags)) op.type = OP_GEMM64;
                // a square hidden layer on the latency lane (the one-step actor's backward tail behind the Euler chain): the chain
                // kernel's variant D does it in about half the time of the generic 16-row kernel
                if (op.type == OP_GEMM && use_chain && t.N == t.K && t.N == cfg.actor_hidden[0] && t.M % 16 == 0 &&
                    t.lda == t.K && t.ldb == t.K && t.ldc == t.N && prev.out_p == t.N) {
                    ChainArgs a{};
                    a.A = t.A; a.Wf = t.B; a.C = t.C; a.Zprev = t.Zprev; a.bias = nullptr;
                    a.M = t.M; a.ad = cfg.act_dim; a.ap = pad16(cfg.act_dim);
                    a.variant = 3;
                    Op co = chain_op(a);
                    co.reads = op.reads; co.writes = op.writes;
                    push(pr, co);
                } else
                push(pr, op);
            }
        }
        // level alignment: start this chain together with a sibling chain so their per-level tasks share launches
        if (align_with)
            for (size_t i = first_op; i < pr.ops.size(); ++i)
                if (pr.ops[i].type != OP_WGRAD) { pr.ops[i].reads.push_back(align_with); break; }
    }

    // ---------------------------------------------------------------------------------------
    // scheduling + launch tables + graph capture
    // ---------------------------------------------------------------------------------------
    // The launches that merge the ops of a level are bound where they are formed, by one helper per family, from what the Launch holds by
    // then: its tables, counts, grid and host task copies.  (An agent group binds its fused launches with the first two.)
    // OP_GEMM: the 16-row kernel; its K > 512 and Euler-prologue instantiations where a task of the launch needs them
    void bind_gemm16(Launch& L) const {
        bool kbig = false, euler = false;
        size_t lds = 0;
        for (const GemmTask& t : L.h_gemm) {
            kbig |= t.K > 512;
            euler |= (t.flags & (GF_A_EULER0 | GF_HEAD_PART | GF_A_LOSSACT)) != 0;
            lds = std::max(lds, ((size_t)16 * (t.K + 4) + 1024 + 1280) * sizeof(float));
        }
        const Geo g(dim3(L.grid), dim3(FQL_THREADS), lds);
        auto table = [&](auto kernel) { return tl_last(bind(kernel, g, (const GemmTask*)L.table, L.ntasks, -1)); };
        L.k = euler ? (kbig ? table(fql_gemm16_euler_kernel<true>) : table(fql_gemm16_euler_kernel<false>))
                    : (kbig ? table(fql_gemm16_kernel<true>) : table(fql_gemm16_kernel<false>));
    }
    // OP_GEMM64, the level's side-lane launch: 64 x 64 tile tasks take fql_side_big_kernel, precision = 2 the split bodies; the tasks travel
    // as the kernel argument when they fit its capacities and FQL_KERNARG_TASKS does not forbid it, else the kernel reads the four tables
    void bind_side(Launch& L, size_t lds) const {
        bool big = false;
        for (const GemmTask& t : L.h_gemm) big |= t.tmt == 2;
        const bool split = cfg.precision == 2;
        const Geo g(dim3(L.grid), dim3(FQL_THREADS), lds);
        const std::unique_ptr<SideArgs> a = ka_tasks ? ka_side_args(L) : nullptr;
        L.ka = a != nullptr;
        auto ka = [&](auto kernel) { return tl_in(bind(kernel, g, *a), offsetof(SideArgs, f) + offsetof(SideFront, tl)); };
        auto table = [&](auto kernel) {
            return tl_last(bind(kernel, g, (const GemmTask*)L.table, L.ntasks, (const WgradTask*)L.table_w, L.n_w, (const LnBwdTask*)L.table_l, L.n_l,
                                L.tile_w, L.tile_l, (const MiscTask*)L.table_m, L.tile_m, -1));
        };
        if (a) L.k = big ? ka(fql_side_big_ka_kernel) : split ? ka(fql_side_split_ka_kernel) : ka(fql_side_ka_kernel);
        else L.k = big ? table(fql_side_big_kernel) : split ? table(fql_side_split_kernel) : table(fql_side_kernel);
    }
    // OP_CONV, OP_CONV_U8, OP_CONV_WGRAD, OP_CONV_WRED: the arg structs of the level in L.table.  pool_fused: the stack's max-pool runs inside
    // the convolution kernel
    void bind_conv(Launch& L, bool pool_fused, size_t lds) const {
        const bool split = cfg.precision == 2;
        const Geo g(dim3(L.grid), dim3(FQL_THREADS), lds);
        auto conv = [&](auto kernel) { return bind(kernel, g, (const ConvArgs*)L.table, L.ntasks); };
        if (L.type == OP_CONV_WRED) L.k = bind(fql_conv_wgrad_reduce_kernel, L.grid, (const ConvWredArgs*)L.table, L.ntasks);
        else if (L.type == OP_CONV_WGRAD)
            L.k = split ? bind(fql_conv_wgrad_split_kernel, g, (const ConvWgradArgs*)L.table, L.ntasks)
                        : bind(fql_conv_wgrad_kernel, g, (const ConvWgradArgs*)L.table, L.ntasks);
        else if (pool_fused) L.k = split ? conv(fql_conv3x3_pool_split_kernel) : conv(fql_conv3x3_pool_kernel);
        else if (L.type == OP_CONV) L.k = split ? conv(fql_conv3x3_split_kernel) : conv(fql_conv3x3_kernel);
        else L.k = split ? conv(fql_conv3x3_u8_split_kernel) : conv(fql_conv3x3_u8_kernel);
    }
    // OP_CONV_WPREP: n tasks (one encoder pass's, or those of the passes of a level), four workgroups each
    static Bound bind_wprep(const ConvWprepTask* tasks, int n) {
        return bind(fql_conv_wprep_kernel, Geo(dim3(4, n), dim3(FQL_THREADS), 0), tasks);
    }

    // schedule(), the steps of which follow in the order it calls them: levels, launches (one former per family), MACs, waits.
    void schedule(Program& pr, std::vector<void*>& owner) {
        assign_levels(pr);
        form_launches(pr, owner);
        for (const Op& o : pr.ops)   // algorithmic MACs per launch (real, unpadded layer widths are within 1 % of these)
            if (o.launch >= 0) pr.launches[o.launch].macs += op_macs(o);
        cross_lane_waits(pr);
        if (getenv("FQL_DUMP")) dump_program(pr);
        check_lane_edges(pr);
    }

    // list scheduling: level = 1 + max level of every op this one conflicts with (RAW, WAW, WAR)
    static void assign_levels(Program& pr) {
        std::map<const void*, int> last_writer;               // buffer -> op index of last writer
        std::map<const void*, std::vector<int>> readers;      // buffer -> ops reading it since that write
        for (int oi = 0; oi < (int)pr.ops.size(); ++oi) {
            Op& op = pr.ops[oi];
            op.deps.clear();
            for (const void* r : op.reads) {
                auto it = last_writer.find(r);
                if (it != last_writer.end()) op.deps.push_back(it->second);
            }
            for (const void* w : op.writes) {
                auto it = last_writer.find(w);
                if (it != last_writer.end()) op.deps.push_back(it->second);
                auto ir = readers.find(w);
                if (ir != readers.end()) for (int r : ir->second) if (r != oi) op.deps.push_back(r);
            }
            int lv = 0;
            for (int d : op.deps) lv = std::max(lv, pr.ops[d].level + 1);
            op.level = lv;
            for (const void* r : op.reads) readers[r].push_back(oi);
            for (const void* w : op.writes) {
                last_writer[w] = oi;
                readers.erase(w);
            }
        }
        // The folds of the encoders' weight-gradient partials (27 tiny tasks, one launch per convolution level = 9 launches of ~16 us in the
        // middle of the backward pass) are needed by nothing but their module's Adam launch: as late as possible they share one launch per module.
        std::vector<std::vector<int>> cons(pr.ops.size());
        for (int oi = 0; oi < (int)pr.ops.size(); ++oi)
            for (int d : pr.ops[oi].deps) cons[d].push_back(oi);
        for (int oi = (int)pr.ops.size() - 1; oi >= 0; --oi) {
            Op& op = pr.ops[oi];
            if (op.type != OP_CONV_WRED) continue;
            int lv = 1 << 30;
            for (int c : cons[oi]) lv = std::min(lv, pr.ops[c].level - 1);
            if (cons[oi].empty()) {   // (the optimizer is another program: the end of this one)
                lv = 0;
                for (const Op& o2 : pr.ops) lv = std::max(lv, o2.level);
            }
            if (lv > op.level) op.level = lv;
        }
    }

    // The launch family an op type merges into, which is also its place in the launch order of a (level, lane): the side-lane riders of a
    // level share ONE launch with its gemm64 tiles (fql_side_kernel), at OP_GEMM64's place; every other type is a family of its own.
    static OpType family(OpType t) {
        return t == OP_WGRAD || t == OP_LNBWD || t == OP_POSTOS || t == OP_LOSS_CRITIC || t == OP_LOSS_Q || t == OP_LOSS_BC ? OP_GEMM64 : t;
    }
    // ... and how many of the n ops of a cell go into one launch: all of a merging family, the dQ/da tasks four at a time (the kernel takes
    // them as its argument), one of everything else
    static size_t per_launch(OpType fam, size_t n) {
        const bool merges = fam == OP_GEMM || fam == OP_GEMM64 || fam == OP_CONV || fam == OP_CONV_U8 || fam == OP_CONV_WGRAD || fam == OP_CONV_WRED || fam == OP_CONV_WPREP;
        return merges ? n : fam == OP_DGRAD0 ? 4 : 1;
    }
    using Cell = std::vector<Op*>;   // ops of one (level, lane, family), in op order
    // Launch order: level ascending, then lane, then family in enum order, then op order within the family.
    void form_launches(Program& pr, std::vector<void*>& owner) {
        pr.launches.clear();
        for (bool& b : pr.lane_used) b = false;
        std::map<std::tuple<int, int, int>, Cell> cells;
        for (Op& op : pr.ops) {
            op.launch = -1;
            if (op.lane >= 0 && op.lane < FQL_LANES) cells[{op.level, op.lane, (int)family(op.type)}].push_back(&op);
        }
        for (const auto& [key, ops] : cells) {
            const OpType fam = (OpType)std::get<2>(key);
            const size_t n = per_launch(fam, ops.size());
            for (size_t i = 0; i < ops.size(); i += n) {
                const Cell part(ops.begin() + i, ops.begin() + std::min(ops.size(), i + n));
                for (Op* o : part) o->launch = (int)pr.launches.size();
                pr.lane_used[part[0]->lane] = true;
                pr.launches.push_back(form(fam, part, owner));
            }
        }
    }
    // one former per family: the ops of a launch in, the launch out - task fields, table upload and bind_* call inside
    Launch form(OpType fam, const Cell& ops, std::vector<void*>& owner) {
        switch (fam) {
        case OP_GEMM: return form_gemm16(ops, owner);
        case OP_GEMM64: return form_side(ops, owner);
        case OP_CONV: case OP_CONV_U8: case OP_CONV_WGRAD: case OP_CONV_WRED: return form_conv(ops, owner);
        case OP_DGRAD0: return form_dgrad0(ops);
        case OP_CONV_WPREP: if (ops.size() > 1) return form_wprep(ops, owner); [[fallthrough]];   // a lone one keeps its own bound launch
        default: return form_single(*ops[0]);
        }
    }
    void* upload(std::vector<void*>& owner, const void* src, size_t bytes) {   // a task table in device memory
        void* d = dalloc(owner, bytes / sizeof(float) + 4);
        if (bytes) HIP_CHECK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        return d;
    }
    static Launch form_single(const Op& o) {   // a launch of its own, bound where the op was emitted
        Launch L(o.type, o.lane);
        L.k = o.k;
        return L;
    }

    // The tile policies of the side launch.
    // 32 x 64 tiles while a level is a latency chain (B = 256: 1.5 workgroups per CU), 64 x 64 once a task alone
    // brings >= 128 of them (M >= 1024: +2 % at B = 1024); returns the tile's rows / 32 (split bodies are 32-row tiles)
    int side_ri(const GemmTask& t) const { return cfg.precision != 2 && t.M >= 1024 && t.M % 64 == 0 ? 2 : 1; }
    // tile shape of the 32-row tasks of a launch: 32 x 64 unless 32 x 32 tiles deal out more evenly over the CUs
    // (e.g. 384 tiles of 32 x 64 = two tile times on half the CUs; 768 of 32 x 32 = three half-size tiles everywhere); returns the tile's columns / 32
    int side_nj(const Cell& g, const Cell& w, const Cell& l) const {
        int t64 = 0;
        double other = 0.0;   // in units of a 32 x 32 x 512 tile
        for (const Op* o : g) {
            const GemmTask& t = o->gemm;
            if (side_ri(t) == 2) other += 4.0 * (t.M / 64) * (t.N / 64) * t.K / 512.0;
            else t64 += (t.M / 32) * (t.N / 64);
        }
        for (const Op* o : w) other += 0.5 * (o->wgrad.Kin / 16) * ((o->wgrad.N + 63) / 64) * o->wgrad.M / 256.0;
        for (const Op* o : l) other += 0.05 * o->ln.M;
        const int ncu = std::max(1, num_cus);
        const double m64 = 2.0 * ((t64 + ncu - 1) / ncu) + other / ncu, m32 = 1.0 * ((2 * t64 + ncu - 1) / ncu) + other / ncu;
        return t64 > 0 && m32 < m64 && !wide_tiles ? 1 : 2;
    }
    // XCD-aware tile order of a 32-row task (ntn set): gm x gn = 8 blocks of the tile grid, fewest panel fetches; returns gm, 0 = none fits
    static int side_xg(const GemmTask& t) {
        const int ntm = t.M / 32;
        // gm row groups x gn column groups: an A row panel is fetched by gn XCDs, a B column panel by gm -> fewest panel bytes
        // (measured on the whole update: the rule's choice 3075, gm forced to 4: 3001-3061, 8: 2864-3026, 1: 2967-3040, no XCD order: 3025)
        int xg = 0;
        double best = 1e30;
        for (int gm : {1, 2, 4, 8}) {
            const int gn = 8 / gm;
            if (ntm % gm || t.ntn % gn) continue;
            const double cost = (double)gn * t.M + (double)gm * t.N;
            if (cost < best) { best = cost; xg = gm; }
        }
        return xg;
    }
    // OP_GEMM64 and its riders: the gemm64 tiles of the cell, then its weight-gradient, LayerNorm-backward and loss / metric tasks
    Launch form_side(const Cell& ops, std::vector<void*>& owner) {
        Cell sel, selw, sell, selm;
        for (Op* o : ops) (o->type == OP_GEMM64 ? sel : o->type == OP_WGRAD ? selw : o->type == OP_LNBWD ? sell : selm).push_back(o);
        Launch L(OP_GEMM64, ops[0]->lane);
        const int nj = side_nj(sel, selw, sell);
        int ri = 1;
        int tile = 0;
        for (const Op* o : sel) {
            GemmTask t = o->gemm;
            t.tmt = side_ri(t);
            ri = std::max(ri, t.tmt);
            t.wk = t.tmt == 2 ? 2 : nj;          // MFMA column tiles per wave: tile = 32 x (32 wk)
            t.ntn = t.N / (32 * t.wk); t.tile0 = tile;
            t.xg = t.tmt == 1 && tile % 8 == 0 ? side_xg(t) : 0;
            tile += (t.M / (32 * t.tmt)) * t.ntn;
            L.h_gemm.push_back(t);
        }
        L.tile_w = tile;
        const int wkt = cfg.precision == 2 ? FQL_WGRAD_KT_SPLIT : FQL_WGRAD_KT;   // weight-gradient tile height of the body this launch runs
        int tilew = 0;
        for (const Op* o : selw) {
            WgradTask t = o->wgrad;
            t.ntn = (t.N + 63) / 64; t.tile0 = tilew;
            tilew += ((t.Kin + wkt - 1) / wkt) * t.ntn;
            L.h_wgrad.push_back(t);
        }
        L.tile_l = L.tile_w + tilew;
        int tilel = 0;
        for (const Op* o : sell) {
            LnBwdTask t = o->ln;
            t.ntiles_rows = (t.M + 3) / 4; t.tile0 = tilel;
            tilel += t.ntiles_rows + (t.dgamma ? t.H / 16 : 0);
            L.h_ln.push_back(t);
        }
        L.tile_m = L.tile_l + tilel;
        for (const Op* o : selm) {
            MiscTask t{};
            if (o->type == OP_POSTOS) { t.kind = MISC_POSTOS; t.po = o->postos; }
            else if (o->type == OP_LOSS_CRITIC) { t.kind = MISC_LOSS_CRITIC; t.lc = o->lc; }
            else if (o->type == OP_LOSS_Q) { t.kind = MISC_LOSS_Q; t.lq = o->lq; }
            else { t.kind = MISC_LOSS_BC; t.lb = o->lb; }
            L.h_misc.push_back(t);
        }
        L.grid = L.tile_m + (int)L.h_misc.size();
        L.ntasks = (int)L.h_gemm.size(); L.n_w = (int)L.h_wgrad.size(); L.n_l = (int)L.h_ln.size();
        const size_t wlds = cfg.precision == 2 ? (size_t)(4 * 4 * 64 * 4 + 4 * 64) : (size_t)FQL_WGRAD_LDS_FLOATS;   // 16- / 32-input tiles
        size_t lds = sizeof(float) * (sel.empty() ? wlds
                                 : ri == 2 ? (size_t)(2 * (32 * ri + 64) * 68 + 256)
                                 : cfg.precision == 2 ? (size_t)FQL_TILE_SPLIT_LDS_FLOATS(nj)
                                 : nj == 1 ? (size_t)(2 * 32 * 68 + 2 * 64 * 36 + 128) : (size_t)(2 * 32 * 68 + 2 * 64 * 68 + 128));
        lds = std::max(lds, sizeof(float) * (selw.empty() ? (size_t)0 : wlds));
        L.table = upload(owner, L.h_gemm.data(), L.h_gemm.size() * sizeof(GemmTask));
        L.table_w = upload(owner, L.h_wgrad.data(), L.h_wgrad.size() * sizeof(WgradTask));
        L.table_l = upload(owner, L.h_ln.data(), L.h_ln.size() * sizeof(LnBwdTask));
        L.table_m = upload(owner, L.h_misc.data(), L.h_misc.size() * sizeof(MiscTask));
        bind_side(L, lds);
        return L;
    }
    // OP_CONV, OP_CONV_U8, OP_CONV_WGRAD, OP_CONV_WRED: every convolution-family op of a cell shares ONE launch (e.g. the same layer of the
    // four encoder passes): arg structs in an HBM table, workgroup ranges by tile0
    Launch form_conv(const Cell& sel, std::vector<void*>& owner) {
        Launch L(sel[0]->type, sel[0]->lane);
        L.ntasks = (int)sel.size();
        int tile = 0;
        size_t lds = 0;
        bool pool_fused = false;
        if (L.type == OP_CONV || L.type == OP_CONV_U8) {
            std::vector<ConvArgs> tb;
            long long nb_all = 0;
            for (const Op* o : sel) nb_all += (long long)o->conv.N * (o->conv.H / o->conv.R);
            // persistent uint8 kernel: its 162 registers (launch bound 3 waves per SIMD) allow three workgroups per CU; exactly that many are launched (a fourth
            // round of workgroups would run alone) and dealt to the tasks in proportion to their row blocks (the one-step pass
            // holds [obs ; next_obs], twice the images of the others), rounded DOWN so the total never exceeds the resident set
            constexpr int u8_per_cu = 3;
            for (const Op* o : sel) {
                ConvArgs a = o->conv;
                const int nb = a.N * (a.H / a.R);
                a.tile0 = tile;
                // float layers: a workgroup per row block (persistent float layers were measured at +-1 %)
                a.nwg = L.type == OP_CONV_U8 ? std::min(nb, std::max(1, (int)(((long long)u8_per_cu * num_cus * nb) / nb_all))) : nb;
                if (a.parg) {   // convolution + max-pool in one kernel: a workgroup per (image, pooled row pair)
                    a.nwg = a.N * ((a.H + 3) / 4);
                    pool_fused = true;
                    lds = std::max(lds, (size_t)FQL_CONV_POOL_LDS_FLOATS(a.W, a.Ci, a.Co) * sizeof(float));
                } else if (pool_fused) invalid("internal: a launch mixes fused and plain convolutions");
                tile += a.nwg;
                lds = std::max(lds, ((size_t)(a.R + 2) * (a.W + 2) * (a.Ci + 4) + (size_t)a.Co * (9 * a.Ci + 4)) * sizeof(float));
                if (L.type == OP_CONV && cfg.precision == 2) lds = std::max(lds, (size_t)FQL_CONV_SPLIT_LDS_WORDS(a.R, a.W, a.Ci, a.Co) * sizeof(float));
                tb.push_back(a);
            }
            L.table = upload(owner, tb.data(), tb.size() * sizeof(ConvArgs));
        } else if (L.type == OP_CONV_WGRAD) {
            std::vector<ConvWgradArgs> tb;
            for (const Op* o : sel) {
                ConvWgradArgs a = o->cw;
                a.tile0 = tile; a.nwg = o->cw_grid;
                tile += a.nwg;
                lds = std::max(lds, ((size_t)(a.R + 2) * (a.W + 2) * (a.Ci + 4) + (size_t)a.R * a.W * (a.Co + 4)) * sizeof(float));
                tb.push_back(a);
            }
            L.table = upload(owner, tb.data(), tb.size() * sizeof(ConvWgradArgs));
        } else {
            std::vector<ConvWredArgs> tb;
            for (const Op* o : sel) {
                ConvWredArgs a = o->cwr;
                a.tile0 = tile;
                tile += ((9 * a.Ci + 1) * a.Co + 63) / 64;
                tb.push_back(a);
            }
            L.table = upload(owner, tb.data(), tb.size() * sizeof(ConvWredArgs));
        }
        L.grid = tile;
        bind_conv(L, pool_fused, lds);
        return L;
    }
    // OP_DGRAD0: up to four members' dQ/da tasks of a level, as the kernel's argument
    Launch form_dgrad0(const Cell& sel) {
        Launch L(OP_DGRAD0, sel[0]->lane);
        Dgrad0Args a{};
        a.col0 = sel[0]->gemm.i1;
        for (const Op* o : sel) {
            if (o->gemm.M != sel[0]->gemm.M || o->gemm.i1 != sel[0]->gemm.i1) invalid("internal: dQ/da tasks of one level differ in shape");
            a.t[a.ntasks++] = o->gemm;
        }
        L.k = bind(fql_dgrad0_kernel, a.ntasks * (sel[0]->gemm.M / 16), a);
        return L;
    }
    // OP_CONV_WPREP, more than one in a cell: the encoder passes of one level refresh their LDS-layout weight copies in ONE launch
    Launch form_wprep(const Cell& sel, std::vector<void*>& owner) {
        int tot = 0;
        for (const Op* o : sel) tot += o->wprep_n;
        ConvWprepTask* all = (ConvWprepTask*)dalloc(owner, (size_t)tot * sizeof(ConvWprepTask) / sizeof(float) + 4);
        int at = 0;
        for (const Op* o : sel) {
            HIP_CHECK(hipMemcpy(all + at, o->wprep_tasks, (size_t)o->wprep_n * sizeof(ConvWprepTask), hipMemcpyDeviceToDevice));
            at += o->wprep_n;
        }
        Launch L(OP_CONV_WPREP, sel[0]->lane);
        L.k = bind_wprep(all, tot);
        return L;
    }
    // OP_GEMM: the 16-row tasks of a cell, from a table
    Launch form_gemm16(const Cell& sel, std::vector<void*>& owner) {
        Launch L(OP_GEMM, sel[0]->lane);
        L.ntasks = (int)sel.size();
        int tile = 0;
        for (const Op* o : sel) {
            GemmTask t = o->gemm;
            t.wk = (t.N <= 16) ? 4 : 2;
            // (two 16-row tiles per workgroup sharing each B fragment were tried on the throughput lane: not kept)
            t.tmt = 1;
            t.ntn = (t.N / 16 + (4 / t.wk) - 1) / (4 / t.wk);
            t.tile0 = tile;
            tile += (t.M / 16) * t.ntn;
            L.h_gemm.push_back(t);
        }
        L.table = upload(owner, L.h_gemm.data(), L.h_gemm.size() * sizeof(GemmTask));
        L.grid = tile;
        bind_gemm16(L);
        return L;
    }

    // algorithmic multiply-accumulates of one op
    static double op_macs(const Op& o) {
        if (o.type == OP_GEMM || o.type == OP_GEMM64 || o.type == OP_HEAD_DGRAD) return (double)o.gemm.M * o.gemm.N * o.gemm.K;
        if (o.type == OP_DGRAD0) return (double)o.gemm.M * 16.0 * o.gemm.K;
        if (o.type == OP_WGRAD) return (double)o.wgrad.M * o.wgrad.Kin * o.wgrad.N;
        if (o.type == OP_CHAIN) return o.macs;
        if (o.type == OP_CONV || o.type == OP_CONV_U8) return (double)o.conv.N * o.conv.H * o.conv.W * 9.0 * (o.conv.transposed ? o.conv.Ci : o.conv.Ci_real) * o.conv.Co;
        if (o.type == OP_CONV_WGRAD) return (double)o.cw.N * o.cw.H * o.cw.W * 9.0 * o.cw.Ci_real * o.cw.Co;
        return 0.0;
    }
    // cross-lane edges: a launch waits for the latest launch of the other lane it depends on (lane streams
    // are in-order, so that covers the earlier ones); skip waits already implied by an earlier wait.
    static void cross_lane_waits(Program& pr) {
        std::vector<int> need(pr.launches.size() * FQL_LANES, -1);   // [launch][other lane]: the latest launch there it depends on
        for (const Op& o : pr.ops) {
            if (o.launch < 0) continue;
            for (int d : o.deps) {
                const int dl = pr.ops[d].launch;
                const int ol = pr.launches[dl].lane;
                int& nd = need[o.launch * FQL_LANES + ol];
                if (ol != o.lane) nd = std::max(nd, dl);
            }
        }
        int waited_upto[FQL_LANES][FQL_LANES];  // [waiting lane][other lane]: highest launch index already waited for
        for (auto& r : waited_upto) for (int& v : r) v = -1;
        for (int li = 0; li < (int)pr.launches.size(); ++li) {
            Launch& L = pr.launches[li];
            for (int ol = 0; ol < FQL_LANES; ++ol) {
                const int nd = need[li * FQL_LANES + ol];
                if (nd <= waited_upto[L.lane][ol]) continue;
                L.waits.push_back(nd);
                pr.launches[nd].record_after = true;
                waited_upto[L.lane][ol] = nd;
            }
        }
    }
    void dump_program(const Program& pr) const {   // FQL_DUMP: the launches with their level, waits and ops
        std::vector<int> level(pr.launches.size(), -1);
        std::vector<std::string> what(pr.launches.size());
        char b[96];
        for (const Op& o : pr.ops) {
            if (o.launch < 0) continue;
            level[o.launch] = o.level;
            if (o.type == OP_GEMM || o.type == OP_GEMM64) snprintf(b, sizeof b, " g%s(%dx%dx%d%s)", o.type == OP_GEMM64 ? "64" : "16", o.gemm.M, o.gemm.N, o.gemm.K, (o.gemm.flags & GF_TRANS_B) ? "T" : "");
            else if (o.type == OP_WGRAD) snprintf(b, sizeof b, " w(%dx%dx%d)", o.wgrad.M, o.wgrad.Kin, o.wgrad.N);
            else if (o.type == OP_LNBWD) snprintf(b, sizeof b, " ln(%d)", o.ln.M);
            else snprintf(b, sizeof b, " t%d", (int)o.type);
            what[o.launch] += b;
        }
        int cnt[FQL_LANES] = {};
        for (int li = 0; li < (int)pr.launches.size(); ++li) {
            const Launch& L = pr.launches[li];
            cnt[L.lane]++;
            fprintf(stderr, "[fql] #%2d level %3d lane %d type %2d ntasks %2d grid %5d waits[", li, level[li], L.lane, (int)L.type, L.ntasks, L.grid);
            for (int w : L.waits) fprintf(stderr, "%d ", w);
            fprintf(stderr, "] :%s\n", what[li].c_str());
        }
        fprintf(stderr, "[fql] launches per lane:");
        for (int l = 0; l < FQL_LANES; ++l) fprintf(stderr, " %d", cnt[l]);
        fprintf(stderr, "\n");
        dump_in_update_reads(pr);
    }
    // FQL_DUMP, second part: per launch, the buffers it reads that an earlier launch of the same program writes - the operands that must be read past
    // the L1 (fql_kernels.h ldx) before the program may drop the acquires between its packets (build_aql).  A buffer is named by the task member that
    // holds it where the op carries a payload, else by its place among the op's reads; `<- #n` is the last earlier launch that writes it.
    void dump_in_update_reads(const Program& pr) const {
        auto member = [](const Op& o, const void* p) -> std::string {
            std::string s;
            auto add = [&](const char* n, const void* q) { if (q == p) { if (!s.empty()) s += '/'; s += n; } };
            if (o.type == OP_GEMM || o.type == OP_GEMM64 || o.type == OP_HEAD_DGRAD) {
                const GemmTask& t = o.gemm;
                add("A", t.A); add("B", t.B); add("bias", t.bias); add("Zprev", t.Zprev); add("aux", t.aux); add("aux2", t.aux2); add("ln_g", t.ln_g);
                add("ln_b", t.ln_b); add("ea_in", t.ea_in); add("evp", t.evp); add("ew", t.ew); add("ew4", t.ew4); add("eb", t.eb);
            } else if (o.type == OP_WGRAD) {
                add("X", o.wgrad.X); add("dZ", o.wgrad.dZ);
            } else if (o.type == OP_LNBWD) {
                const LnBwdTask& t = o.ln;
                add("dY", t.dY); add("Z", t.Z); add("Gv", t.Gv); add("stats", t.stats); add("gamma", t.gamma); add("dq", t.dq); add("wq", t.wq);
            }
            return s;
        };
        std::map<const void*, int> writer;   // buffer -> last launch, so far, that writes it
        size_t oi = 0;
        for (int li = 0; li < (int)pr.launches.size(); ++li) {
            std::string line;
            std::vector<const Op*> mine;
            for (const Op& o : pr.ops) if (o.launch == li) mine.push_back(&o);
            for (const Op* o : mine)
                for (size_t ri = 0; ri < o->reads.size(); ++ri) {
                    auto it = writer.find(o->reads[ri]);
                    if (it == writer.end()) continue;
                    char b[96];
                    const std::string m = member(*o, o->reads[ri]);
                    snprintf(b, sizeof b, " t%d.%s%s<-#%d", (int)o->type, m.empty() ? "r" : m.c_str(), m.empty() ? std::to_string(ri).c_str() : "", it->second);
                    line += b;
                }
            for (const Op* o : mine) for (const void* w : o->writes) writer[w] = li;
            fprintf(stderr, "[fql] #%2d type %2d in-update reads:%s\n", li, (int)pr.launches[li].type, line.empty() ? " none" : line.c_str());
        }
        (void)oi;
    }
    // Two FORKED lanes (>= 1; lane 0 is the capture's origin stream) must not wait on each other in both directions: the HIP
    // runtime bundled with torch 2.10 (ROCm 7.0) walks the resulting cycle of parallel capture streams forever in
    // hip::Stream::EndCapture (a segmentation fault by stack exhaustion; diagnosed with rocgdb, profiles/r02_capture_crash.txt).
    // The default programs keep such edges one-directional by construction; placement overrides that do not are refused.
    static void check_lane_edges(const Program& pr) {
        bool edge[FQL_LANES][FQL_LANES] = {};
        for (const Launch& L : pr.launches)
            for (int w : L.waits) edge[pr.launches[w].lane][L.lane] = true;
        for (int a = 1; a < FQL_LANES; ++a)
            for (int b = a + 1; b < FQL_LANES; ++b)
                if (edge[a][b] && edge[b][a])
                    invalid("lane placement makes lanes %d and %d wait on each other in both directions: not capturable on this HIP runtime "
                            "(hipStreamEndCapture recursion); move one of the passes", a, b);
    }

    // One launch of a program on stream s: what was bound where the launch was formed (Launch::k), as it stands but for the timeline id
    // (tl, diagnostics build only, -1 = none) and the one run-time argument of the programs, the sampling call's cfg.
    // Per-launch profiling (fql_profile_update): when set, the next launch carries these two events ON ITS DISPATCH
    // (hipExtLaunchKernel): their elapsed time is the dispatch's own begin-to-end time, the quantity a rocprofv3 kernel trace reports.
    hipEvent_t prof_a = nullptr, prof_b = nullptr;
    // the arguments of launch L as issued: a (FQL_BOUND_BYTES) receives L.k.args with tl and sample_cfg written
    void issue_args(const Launch& L, int tl, unsigned char* a) const {
        const Bound& k = L.k;
        if (!k.fn) throw HipError{"internal: op type " + std::to_string((int)L.type) + " carries no bound launch"};
        std::memcpy(a, k.args.data(), k.args.size());
        if (k.tl_at >= 0) std::memcpy(a + k.tl_at, &tl, sizeof tl);
        // a run-time float: the cached sampling program holds every other argument
        if (L.type == OP_IQLD_CFG) std::memcpy(a + offsetof(IqldCfgStepArgs, cfg), &sample_cfg, sizeof sample_cfg);
    }
    void issue(const Launch& L, hipStream_t s, int tl) {
        alignas(16) unsigned char a[FQL_BOUND_BYTES];
        issue_args(L, tl, a);
        launch_bound(L.k, a, s, prof_a, prof_b);
    }
    // the timeline id of a launch of `pr` (diagnostics build only: the launches of prog_full)
    int tl_of(const Program& pr, const Launch& L) const { return &pr == &prog_full ? (int)(&L - pr.launches.data()) : -1; }
    // a program's launches through issue_lanes (ls == nullptr: every launch on s0), logged under FQL_TRACE
    void run_launches(Program& pr, hipStream_t s0, const hipStream_t* ls = nullptr, bool fork = true) {
        static const bool trace_l = getenv("FQL_TRACE") != nullptr;
        issue_lanes(pr, s0, ls, fork, [&](const Launch& L, hipStream_t s) {
            if (trace_l) {
                fprintf(stderr, "[fql] launch %d type %d lane %d grid %d waits %zu:", (int)(&L - pr.launches.data()), (int)L.type, L.lane, L.grid, L.waits.size());
                for (int w : L.waits) fprintf(stderr, " %d(lane %d)", w, pr.launches[w].lane);
                fprintf(stderr, "\n");
            }
            issue(L, s, tl_of(pr, L));
        });
    }
    // what issue() hands to the runtime for each launch of `pr`, in order, as the AQL path takes it (fql_aql.h): a plain copy of Launch::k
    std::vector<AqlDispatch> dispatches(const Program& pr) const {
        std::vector<AqlDispatch> out;
        alignas(16) unsigned char a[FQL_BOUND_BYTES];
        for (const Launch& L : pr.launches) {
            issue_args(L, tl_of(pr, L), a);
            const Bound& k = L.k;
            out.push_back(AqlDispatch{k.fn, {k.grid[0], k.grid[1], k.grid[2]}, {k.block[0], k.block[1], k.block[2]}, k.lds, std::vector<uint8_t>(a, a + k.args.size())});
        }
        return out;
    }

    // The program as AQL packet templates for the engine's own HSA queues (fql_aql.h): one queue per lane, the barrier bit inside a lane,
    // completion signal -> barrier-AND packet across lanes, into pr.aql.  Left off (pr.aql.ok = false, the captured graph runs) when the HSA
    // runtime does not come up or FQL_AQL=0.
    const bool aql_acquire = aql_acquire_env();
    static bool l1_independent(const Program& pr) {
        for (const Launch& L : pr.launches)
            if (!l1_independent_kernel(L.k.fn) || L.type == OP_IQLD_CFG) return false;   // (OP_IQLD_CFG: the one launch with an issue-time word)
        return !pr.launches.empty();
    }
    void build_aql(Program& pr) {
        static const bool off = getenv("FQL_AQL") && atoi(getenv("FQL_AQL")) == 0;
        static const bool trace_a = getenv("FQL_TRACE") != nullptr;
        AqlProgram& ap = pr.aql;
        ap = AqlProgram{};
        if (off || visual) return;   // (visual updates gather their frames with HIP launches in front of the program and are device-bound anyway)
        void* kargs = nullptr;
        try {
            if (!aql.up && aql.why.empty()) aql.init(device, (const void*)&fql_create);
            if (!aql.up) throw AqlError{aql.why};
            const std::vector<AqlDispatch> rec = dispatches(pr);
            const size_t n = pr.launches.size();

            std::vector<const AqlKernelInfo*> ki(n);
            std::vector<size_t> koff(n);
            size_t tot = 0;
            for (size_t i = 0; i < n; ++i) {
                ki[i] = &aql.kernel(rec[i].fn);
                if (ki[i]->kernarg_size < rec[i].args.size()) throw AqlError{"recorded arguments exceed the kernel's kernarg segment"};
                koff[i] = tot;
                tot += ((size_t)ki[i]->kernarg_size + 63) & ~(size_t)63;
            }
            std::vector<uint8_t> host(tot);
            for (size_t i = 0; i < n; ++i) AqlRuntime::fill_kernarg(host.data() + koff[i], rec[i], *ki[i]);
            HIP_CHECK(hipMalloc(&kargs, tot));   // device memory: with the blocks in host memory every launch starts 0.7 us later (417 us per update against 355)
            HIP_CHECK(hipMemcpy(kargs, host.data(), tot, hipMemcpyHostToDevice));
            std::vector<int> sig(n, AQL_SIG_NONE);
            int nsig = 0;
            bool used[FQL_AQL_LANES] = {};
            for (const Launch& L : pr.launches) {
                if (L.lane < 0 || L.lane >= FQL_AQL_LANES) throw AqlError{"lane out of range"};
                used[L.lane] = true;
                for (int w : L.waits) if (sig[w] == AQL_SIG_NONE) sig[w] = nsig++;
            }
            if (!used[0]) throw AqlError{"program without a lane 0"};
            int endsig[FQL_AQL_LANES];
            for (int l = 1; l < FQL_AQL_LANES; ++l) endsig[l] = used[l] ? nsig++ : AQL_SIG_NONE;
            // fences between packets: agent scope both ways, as the HIP runtime sets them for kernels of one stream.  Measured (profiles/r03_aql.txt): system scope
            // 416 us per update, agent 355, acquire dropped 336 with the same results over 1300 updates (the invalidate is then left to eviction: not a guarantee,
            // not shipped), release dropped 332 and wrong.
            // An L1-independent program - every launch binds a kernel that reads what earlier launches of the program wrote past the L1 and the
            // scalar cache (l1_independent_kernel), none has words written at issue time - drops the acquire of every kernel packet but the first
            // of each lane: there is nothing stale those caches could serve.  The release stays on every packet.  FQL_AQL_ACQUIRE=1 keeps them.
            constexpr int AG = HSA_FENCE_SCOPE_AGENT, SY = HSA_FENCE_SCOPE_SYSTEM, NO = HSA_FENCE_SCOPE_NONE;
            const int interior = l1_independent(pr) && !aql_acquire ? NO : AG;
            for (int l = 1; l < FQL_AQL_LANES; ++l)
                if (used[l]) {   // the previous update has finished on every lane
                    AqlPacket b = AqlRuntime::barrier_packet(false, NO, NO);
                    b.deps[0] = AQL_SIG_PREV_DONE;
                    ap.lane[l].push_back(b);
                }
            bool first[FQL_AQL_LANES] = {true, true, true, true};
            for (size_t i = 0; i < n; ++i) {
                const Launch& L = pr.launches[i];
                for (size_t w0 = 0; w0 < L.waits.size(); w0 += 5) {
                    AqlPacket b = AqlRuntime::barrier_packet(false, NO, NO);
                    for (size_t j = 0; j < 5 && w0 + j < L.waits.size(); ++j) b.deps[j] = sig[L.waits[w0 + j]];
                    ap.lane[L.lane].push_back(b);
                }
                AqlPacket k = AqlRuntime::kernel_packet(rec[i], *ki[i], (uint64_t)(uintptr_t)kargs + koff[i], true, first[L.lane] ? SY : interior, AG);
                first[L.lane] = false;
                k.complete = sig[i];
                ap.lane[L.lane].push_back(k);
            }
            for (int l = 1; l < FQL_AQL_LANES; ++l)
                if (used[l]) {
                    AqlPacket b = AqlRuntime::barrier_packet(true, NO, AG);
                    b.complete = endsig[l];
                    ap.lane[l].push_back(b);
                }
            {
                AqlPacket b = AqlRuntime::barrier_packet(true, NO, SY);
                int j = 0;
                for (int l = 1; l < FQL_AQL_LANES; ++l) if (used[l]) b.deps[j++] = endsig[l];
                b.complete = AQL_SIG_DONE;
                ap.lane[0].push_back(b);
            }
            aql.ensure_signals(nsig);
            for (int l = 0; l < FQL_AQL_LANES; ++l) if (used[l]) aql.ensure_queue(l);
            ap.nsig = nsig;
            ap.kernargs = kargs;
            ap.ok = true;
            if (trace_a) fprintf(stderr, "[fql] AQL program: %zu launches, packets per lane %zu %zu %zu %zu, %d signals, %zu bytes of kernargs\n", n,
                                 ap.lane[0].size(), ap.lane[1].size(), ap.lane[2].size(), ap.lane[3].size(), nsig, tot);
        } catch (const AqlError& e) {
            if (kargs) hipFree(kargs);
            ap = AqlProgram{};
            if (aql.why.empty()) aql.why = e.msg;
            if (trace_a || getenv("FQL_AQL")) fprintf(stderr, "[fql] AQL path off: %s\n", e.msg.c_str());
        }
    }

    void capture(Program& pr) {
        if (pr.exec) { hipGraphExecDestroy(pr.exec); pr.exec = nullptr; }
        if (pr.graph) { hipGraphDestroy(pr.graph); pr.graph = nullptr; }
        HIP_CHECK(hipStreamSynchronize(stream));
        capture_graph(stream, [&] { run_launches(pr, stream, lane_streams); }, pr.graph, pr.exec);
    }

    // one graph per segment: seg 0 = lane-0 launches up to the last one lane 1 waits on, seg 1 = lane 1, seg 2 = lane 0 up to
    // its first wait on lane 1, seg 3 = the rest of lane 0.  Returns false if the program does not have that shape.
    bool capture_split(Program& pr) {
        int last_needed_by_lane1 = -1, first_lane0_wait = -1;
        for (int li = 0; li < (int)pr.launches.size(); ++li) {
            const Launch& L = pr.launches[li];
            if (L.lane > 1) return false;
            for (int w : L.waits) {
                if (L.lane == 1) last_needed_by_lane1 = std::max(last_needed_by_lane1, w);
                if (L.lane == 0 && first_lane0_wait < 0) first_lane0_wait = li;
            }
        }
        if (last_needed_by_lane1 < 0 || first_lane0_wait < 0 || first_lane0_wait <= last_needed_by_lane1) return false;
        auto seg_of = [&](int li) {
            const Launch& L = pr.launches[li];
            if (L.lane == 1) return 1;
            if (li <= last_needed_by_lane1) return 0;
            return li < first_lane0_wait ? 2 : 3;
        };
        for (int seg = 0; seg < 4; ++seg) {
            Program sub;
            for (int li = 0; li < (int)pr.launches.size(); ++li)
                if (seg_of(li) == seg) { Launch L = pr.launches[li]; L.waits.clear(); L.record_after = false; L.ev = nullptr; L.lane = 0; sub.launches.push_back(L); }
            if (sub.launches.empty()) return false;
            HIP_CHECK(hipStreamSynchronize(stream));
            capture_graph(stream, [&] { run_launches(sub, stream); }, split_graph[seg], split_exec[seg]);
        }
        if (!ev_a) HIP_CHECK(hipEventCreateWithFlags(&ev_a, hipEventDisableTiming));
        if (!ev_b) HIP_CHECK(hipEventCreateWithFlags(&ev_b, hipEventDisableTiming));
        return true;
    }
    void free_split() {
        for (int i = 0; i < 4; ++i) {
            if (split_exec[i]) { hipGraphExecDestroy(split_exec[i]); split_exec[i] = nullptr; }
            if (split_graph[i]) { hipGraphDestroy(split_graph[i]); split_graph[i] = nullptr; }
        }
        split_ok = false;
    }
    // enqueue the split update: s0 carries lane 0, s1 lane 1; on return s1 holds everything bucket 0 of the gradient
    // buffer depends on, s0 everything bucket 1 depends on
    void launch_split(hipStream_t s0, hipStream_t s1) {
        HIP_CHECK(hipGraphLaunch(split_exec[0], s0));
        HIP_CHECK(hipEventRecord(ev_a, s0));
        HIP_CHECK(hipStreamWaitEvent(s1, ev_a, 0));
        HIP_CHECK(hipGraphLaunch(split_exec[1], s1));
        HIP_CHECK(hipEventRecord(ev_b, s1));
        HIP_CHECK(hipGraphLaunch(split_exec[2], s0));
        if (!ev_c) HIP_CHECK(hipEventCreateWithFlags(&ev_c, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(ev_c, s0));          // the Euler chain (the last reader of the BC flow's weights on lane 0) is behind this
        HIP_CHECK(hipStreamWaitEvent(s0, ev_b, 0));
        HIP_CHECK(hipGraphLaunch(split_exec[3], s0));
        split_begun = true;
    }

    // Never throws (fql_destroy runs it, often from a garbage collector): updates of the program's AQL form still on the queues finish
    // first; a queue that has failed was reported by the call that met it, and its buffers are released all the same.
    void free_program(Program& pr) noexcept {
        if (pr.aql.kernargs) {
            try { aql_drain(); } catch (...) {}
            hipFree(pr.aql.kernargs);
        }
        if (pr.exec) hipGraphExecDestroy(pr.exec);
        if (pr.graph) hipGraphDestroy(pr.graph);
        destroy_lane_events(pr);
        pr = Program{};
    }

    // ---------------------------------------------------------------------------------------
    // the training step as a program (agents/fql.py:94-133)
    // ---------------------------------------------------------------------------------------
    void build_step_program(Program& pr, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        const int inp_c = nets[NET_OS].in_p(), inp_b = nets[NET_BC].in_p();
        const int ap = pad16(ad);
        DevState* st = d_state;
        const void* INFO = &st->info[0];
        const void *I_CR = &st->info[0], *I_BC = &st->info[5], *I_Q = &st->info[7], *I_MSE = &st->info[9], *I_ACT = &st->info[4];
        // Lane 0 carries the critical path (prep -> Euler chain -> actor loss -> one-step backward); the rest of
        // the step runs beside it on lane 1 (a second graph branch) and only meets it at the actor loss.
        if (visual) {   // every module encodes the batch images first (agents/fql.py:196-202); the encodings feed prep
            // (data-parallel split program: on lane 0, so that lane 1 depends on lane 0 only through the prep kernel)
            place("enc", split_build ? 0 : 1, true);
            emit_encoder_forward(pr, eb_os);   // [obs ; next_obs]: sample_actions(next_obs) fql.py:25, onestep(obs) fql.py:65,82
            emit_encoder_forward(pr, eb_c);    // critic(obs, .) fql.py:36,70 (same stored encoder and images: one pass)
            emit_encoder_forward(pr, eb_t);    // target_critic(next_obs, .) fql.py:28
            emit_encoder_forward(pr, eb_bc);   // actor_bc_flow(obs, .) fql.py:58 and actor_bc_flow_encoder(obs) fql.py:163 (shared)
        }
        emit_lane = 0;
        {   // batch gather + noise + every network input
            Op op{};
            op.type = OP_PREP;
            PrepArgs pa{d_src, st, seed, B, od, ad, inp_c, inp_b, ap, X_os, X_bc, X_eu, X_c1, X_c2, X_ct, vel, w_rew, w_mask, w_act,
                        fused_euler ? X_e0 : nullptr, nullptr, nullptr, nullptr, nullptr};
            pa.tl = -1; pa.part = 0;
            auto bound = [&](int part) { pa.part = part; return tl_in(bind(fql_prep_kernel, (pa.B + 3) / 4, pa), offsetof(PrepArgs, tl)); };
            // One batch-assembly launch per lane (state agents): the side lane then has no dependency on the critical lane at the
            // start of the update.  (On this runtime a graph branch whose first node waits for a node of the other branch starts
            // only ~16 launches of that branch later: profiles/r02_timeline_concurrent.txt.)
            if (visual) {
                pa.E_c = eb_c.E; pa.E_t = eb_t.E; pa.E_bc = eb_bc.E; pa.E_os = eb_os.E;
                op.reads = {eb_c.E, eb_t.E, eb_bc.E, eb_os.E};
            }
            if (!visual && !split_build) {
                Op a = op, b = op;
                a.k = bound(1);
                a.writes = {X_eu};
                if (fused_euler) a.writes.push_back(X_e0);
                b.k = bound(2);
                b.writes = {X_os, X_bc, X_c1, X_c2, X_ct, vel, w_rew, w_mask, w_act};
                emit_lane = 0; push(pr, a);
                emit_lane = 1; push(pr, b);
                emit_lane = 0;
            } else {
                op.writes = {X_os, X_bc, X_eu, X_c1, X_c2, X_ct, vel, w_rew, w_mask, w_act};
                if (fused_euler) op.writes.push_back(X_e0);
                op.k = bound(0);
                push(pr, op);
            }
        }
        // Three lanes (state agents, single-GPU programs): lane 1 carries only what the one-step actor's backward waits for - the
        // Q-gradient path (one-step forward, critic(obs, actor actions) forward and input-gradient chain) - in light launches;
        // the critic-loss passes, the BC pass, every weight gradient and Adam go to lane 2.  Edges between the two forked
        // lanes run 1 -> 2 only: torch's bundled HIP runtime recurses forever in hipStreamEndCapture when two forked streams wait
        // on each other in BOTH directions (hip::Stream::EndCapture walks the cycle; the system ROCm 7.2 runtime does not).
        const bool lanes3 = !visual && !split_build;
        const int fill_lane = lanes3 ? 2 : 1;
        if (!split_build) fill_lane_full = fill_lane;
        wide_tiles = lanes3;
        place("os", 1, true);
        // one-step actor on [next_obs|eps1 ; obs|z ; obs|eps2]  (agents/fql.py:25,65,82)
        emit_forward(pr, p_os, with_grads, GF_OS_SCATTER, X_ct, X_c2);
        {   // mse metric only (agents/fql.py:82-83); the clipped actions were scattered by the head's epilogue
            Op op{};
            op.type = OP_POSTOS;
            op.postos = PostOsArgs{p_os.out, w_act, X_ct, X_c2, st, B, od, ad, inp_c, ap};
            op.reads = {p_os.out, w_act};
            op.writes = {I_MSE};
            push(pr, op);
        }
        place("c1f", fill_lane, true);   // (forward and loss / backward placed separately: FQL_LANE_c1f / FQL_LANE_c1)
        // critic(obs, actions) with grad params; target critic(next_obs, next_actions)  (fql.py:28,36)
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_c1[e], with_grads);
        // three lanes: the target-critic pass rides on lane 1 (its action block comes from the one-step forward there, and lane 1 is otherwise
        // idle once the Q-gradient path has ended): 2500 -> 2580 updates/s in steady state
        place("ct", lanes3 ? 1 : fill_lane, true);
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_ct[e], false);
        place("c1", fill_lane, true);
        {
            Op op{};
            op.type = OP_LOSS_CRITIC;
            op.lc = LossCriticArgs{p_c1[0].out, p_c1[1].out, p_ct[0].out, p_ct[1].out, w_rew, w_mask,
                                   with_grads ? p_c1[0].dz.back() : nullptr, with_grads ? p_c1[1].dz.back() : nullptr,
                                   st, B, cfg.q_agg, with_grads ? 1 : 0, cfg.discount};
            op.reads = {p_c1[0].out, p_c1[1].out, p_ct[0].out, p_ct[1].out, w_rew, w_mask};
            op.writes = {I_CR};
            if (with_grads) { op.writes.push_back(p_c1[0].dz.back()); op.writes.push_back(p_c1[1].dz.back()); }
            push(pr, op);
        }
        // The critic's weight gradients gate nothing but Adam: they are emitted after the Q-gradient chain, whose levels on lane 1
        // then carry fewer tiles and finish earlier - and with them the one-step actor's backward tail (2127 -> 2170 updates/s;
        // deferring the BC flow's too: 2161, the critic's whole backward chain: 2050).  Not in three-lane programs: there they are on lane 2, out of
        // the Q-gradient path's launches anyway.
        std::vector<Op> late_ops;
        if (!lanes3 && with_grads) defer_wgrads = &late_ops;
        if (with_grads)
            for (int e = 0; e < 2; ++e) emit_backward(pr, p_c1[e], 0, B, true, visual);
        // (not in the data-parallel split program: there lane 1 must finish bucket 0 without waiting for lane 0's tail)
        const bool enc_align = !split_build;
        if (with_grads && visual && !enc_align) {   // the critic's encoder sees the critic loss only (the actor loss uses stored params)
            place("enc", 1, true);
            emit_encoder_backward(pr, eb_c, 0, B, p_c1[0].dx0, p_c1[1].dx0, nets[NET_C0].in_p());
        }
        // BC flow-matching pass (fql.py:52-59), on lane 2 in front of the Q-gradient path.  (Three lanes: emitting it BEHIND the Q-gradient path
        // instead - lane 1 idles from the end of that path to the end of the update while lane 2 carries the longest tail - was tried and not kept.)
        {
            // (three lanes: the BC flow's FORWARD on lane 1 in front of the one-step pass, its loss and backward stay on lane 2 - -0.5 .. -1.0 % per
            // fp32 update in three in-process A/Bs under AQL dispatch, nothing in bf16x3; experiments/lane_sweep.sh)
            place("bcf", lanes3 ? 1 : fill_lane, true);
            emit_forward(pr, p_bc, with_grads);
            place("bc", fill_lane, true);
            {
                Op op{};
                op.type = OP_LOSS_BC;
                op.lb = LossBcArgs{p_bc.out, vel, with_grads ? p_bc.dz.back() : nullptr, st, B, ad, ap, with_grads ? 1 : 0};
                op.reads = {p_bc.out, vel};
                op.writes = {I_BC};
                if (with_grads) op.writes.push_back(p_bc.dz.back());
                push(pr, op);
            }
            defer_wgrads = nullptr;
            if (with_grads) emit_backward(pr, p_bc, 0, B, true, visual);
            if (with_grads && visual && !enc_align) {
                place("enc", 1, true);
                emit_encoder_backward(pr, eb_bc, 0, B, p_bc.dx0, nullptr, nets[NET_BC].in_p());
            }
        }
        // Q term: critic(obs, clip(actor_actions)) with stored params, input-differentiable (fql.py:69-76)
        place("c2", 1, true);
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_c2[e], with_grads);
        {
            Op op{};
            op.type = OP_LOSS_Q;
            // without normalize_q_loss dQ = -1/(2B) is a constant (filled once at workspace build): the input-gradient
            // chain through the critic then does not wait for the Q heads or this kernel
            const bool dyn_dq = with_grads && cfg.normalize_q_loss;
            op.lq = LossQArgs{p_c2[0].out, p_c2[1].out, dyn_dq ? p_c2[0].dz.back() : nullptr,
                              dyn_dq ? p_c2[1].dz.back() : nullptr, st, B, cfg.normalize_q_loss, dyn_dq ? 1 : 0};
            op.reads = {p_c2[0].out, p_c2[1].out};
            op.writes = {I_Q};
            if (dyn_dq) { op.writes.push_back(p_c2[0].dz.back()); op.writes.push_back(p_c2[1].dz.back()); }
            push(pr, op);
        }
        defer_wgrads = nullptr;
        if (with_grads) {
            // two lanes: in phase with the c1 chain (shared launches); three lanes: on its own, as early as its inputs exist
            for (int e = 0; e < 2; ++e) emit_backward(pr, p_c2[e], 0, B, false, true, !lanes3 ? I_CR : nullptr);
        }
        for (Op& w : late_ops) {   // the critic's and the BC flow's weight gradients only after the Q-gradient chain (they gate nothing)
            w.reads.push_back(p_c2[0].dx0); w.reads.push_back(p_c2[1].dx0);
            emit_lane = w.lane;
            push(pr, w);
        }
        // Euler chain through the BC flow (fql.py:155-171): flow_steps sequential forwards
        place("eu", 0, false);
        const int fs = cfg.flow_steps;
        // The last Euler step's target is finished inside the one-step head dgrad's prologue (GF_A_EULFIN: one launch less on the critical lane,
        // bit-identical target).  The 16 partial loads per element lengthen the prologue of all 256 workgroups by most of what the launch boundary
        // saves: -0.45 % per update in both orders of an in-process A/B (experiments/ab_inproc.py; round 2, under the graph's host cost, saw nothing).
        // (A persistent one-launch chain was measured slower than these launches at every batch size: DESIGN.md section 9.)
        euler_finish_fused = with_grads && !cfg.actor_layer_norm && fused_euler && use_chain && fs > 1 && vp_tiles <= 32;
        if (fused_euler && use_chain) emit_euler_chain(pr);
        else if (fused_euler) emit_euler_fused(pr);
        else
        for (int s = 0; s < fs; ++s)
            emit_forward(pr, p_eu, false, GF_EULER | (s == fs - 1 ? GF_EULER_LAST : 0), X_eu, tgt, 1.0f / (float)fs,
                         (float)(s + 1) / (float)fs);
        // The actor-loss gradient is built inside the one-step actor's head dgrad (GF_A_LOSSACT), so the loss kernel only
        // reports scalars and leaves the critical path (it rides on lane 1): 2083 -> 2130 updates/s.
        const bool fuse_la = with_grads && !cfg.actor_layer_norm;
        Op la_op{};
        int la_lane = 0;
        {
            Op op{};
            op.type = OP_LOSS_ACTOR;
            const bool kgrad = with_grads && !fuse_la;
            op.k = bind(fql_loss_actor_kernel, 1, LossActorArgs{p_os.out + (size_t)B * ap, tgt, kgrad ? p_c2[0].dx0 : nullptr,
                                                                kgrad ? p_c2[1].dx0 : nullptr, kgrad ? p_os_bwd.dz.back() : nullptr, st, B, od, ad,
                                                                inp_c, ap, kgrad ? 1 : 0, cfg.alpha});
            op.reads = {p_os.out, tgt, I_BC, I_Q};
            op.writes = {I_ACT};
            if (kgrad) {
                op.reads.push_back(p_c2[0].dx0); op.reads.push_back(p_c2[1].dx0);
                op.writes.push_back(p_os_bwd.dz.back());
            }
            // this kernel, first of lane 2's tail, also takes the edge to the end of lane 1's Q-gradient chain that the critic's Adam
            // behind it needs (write after read of the critic's kernels) - both cross-lane waits of the tail on ONE launch (as in adam_for)
            if (with_grads && !kgrad) { op.reads.push_back(p_c2[0].dx0); op.reads.push_back(p_c2[1].dx0); }
            const int keep = emit_lane;
            if (fuse_la && !split_build) emit_lane = fill_lane;
            if (euler_finish_fused) { la_op = op; la_lane = emit_lane; }   // pushed behind the head dgrad, which now WRITES the target
            else push(pr, op);
            emit_lane = keep;
        }
        if (with_grads) {
            // The one-step actor's weight gradients gate the last Adam launch.  On lane 1 they would queue behind the deferred critic
            // weight gradients and the other two Adam launches; emitted here as ONE launch on lane 0 behind the last dgrad they
            // cost ~10 us of tail instead.  (Lane 1 was the earlier placement.)
            std::vector<Op> os_w;
            defer_wgrads = &os_w;
            const size_t first = pr.ops.size();
            emit_backward(pr, p_os_bwd, B, B, true, visual);
            defer_wgrads = nullptr;
            if (fuse_la) {
                // the head's wgrad (emitted first) reads dA, which the head dgrad (emitted right after it) now PRODUCES:
                // swap them so the scheduler sees the write before the read, then turn the dgrad's A operand into the builder
                float* da = p_os_bwd.dz.back();
                size_t id = first;
                while (id < pr.ops.size() && !(pr.ops[id].type == OP_GEMM && pr.ops[id].gemm.A == da)) ++id;
                if (id >= pr.ops.size() || id > first + 1) invalid("internal: unexpected one-step backward program shape");
                if (id == first + 1) {   // (when the wgrads are emitted in place; deferred ones follow the chain anyway)
                    if (pr.ops[first].type != OP_WGRAD || pr.ops[first].wgrad.dZ != da) invalid("internal: unexpected one-step backward program shape");
                    std::swap(pr.ops[first], pr.ops[first + 1]);
                }
                Op& d = pr.ops[first];
                GemmTask& t = d.gemm;
                t.flags |= GF_A_LOSSACT;
                t.ea_in = p_os.out + (size_t)B * ap; t.evp = tgt; t.i0 = ap; t.i1 = od; t.i2 = ad;
                t.ew = p_c2[0].dx0; t.ew4 = p_c2[1].dx0; t.e_ntp = inp_c;
                t.ea_out = da;
                // the dedicated launch (fql_head_dgrad_kernel) where the task has its shape: a 16-wide contraction into multiples of 64 columns
                if (t.K == 16 && t.N % 64 == 0 && t.M % 16 == 0 && (t.flags & GF_TRANS_B) && (t.flags & GF_GELUGRAD) && !(t.flags & (GF_BIAS | GF_RELUGRAD | GF_A_LN)) &&
                    cfg.precision != 1)
                    d.type = OP_HEAD_DGRAD;
                t.f0 = cfg.alpha * 2.0f / (float)(B * ad);
                d.reads.erase(std::remove(d.reads.begin(), d.reads.end(), (const void*)da), d.reads.end());
                for (const void* r : {(const void*)p_os.out, (const void*)tgt, (const void*)p_c2[0].dx0, (const void*)p_c2[1].dx0}) d.reads.push_back(r);
                d.writes.push_back(da);
                if (euler_finish_fused) {
                    const Net& nb = nets[NET_BC];
                    t.flags |= GF_A_EULFIN;
                    t.aux = Abuf[(fs - 1) & 1]; t.aux2 = Vpart; t.eb = P + nb.layers[nb.nl() - 1].b; t.f1 = 1.0f / (float)fs; t.ln_width = vp_tiles;
                    d.reads.erase(std::remove(d.reads.begin(), d.reads.end(), (const void*)tgt), d.reads.end());
                    for (const void* r : {(const void*)Abuf[(fs - 1) & 1], (const void*)Vpart, (const void*)(P + nb.layers[nb.nl() - 1].w)}) d.reads.push_back(r);   // (head bias: WAR against Adam)
                    d.writes.push_back(tgt);
                }
                if (d.type == OP_HEAD_DGRAD) d.k = bind(fql_head_dgrad_kernel, (t.M / 16) * (t.N / 64), t);   // (the task is complete only here)
            }
            if (euler_finish_fused) {   // the metric kernel reads the target the head dgrad has just written
                const int keep = emit_lane;
                emit_lane = la_lane;
                push(pr, la_op);
                emit_lane = keep;
            }
            // (Three lanes: sending each layer's weight gradient to lane 2, idle by the time the tail runs, as soon as its dz exists was
            // tried and not kept.)
            for (Op& w : os_w) {
                w.reads.push_back(p_os_bwd.dz[0]);   // after the last dgrad: all five in one launch
                emit_lane = 0;
                push(pr, w);
            }
            emit_lane = 0;
        }
        if (with_grads && visual) {   // the obs half of the [obs ; next_obs] pass
            place("enc", split_build ? 0 : 1, true);
            emit_encoder_backward(pr, eb_os, 0, B, p_os_bwd.dx0, nullptr, nets[NET_OS].in_p());
            if (enc_align) {   // all three encoder backward passes level-aligned with the last one: their ops share launches
                emit_encoder_backward(pr, eb_c, 0, B, p_c1[0].dx0, p_c1[1].dx0, nets[NET_C0].in_p(), p_os_bwd.dx0);
                emit_encoder_backward(pr, eb_bc, 0, B, p_bc.dx0, nullptr, nets[NET_BC].in_p(), p_os_bwd.dx0);
            }
        }
        if (!with_grads) emit(pr, OP_FINALIZE, finalize_launch(0), {I_CR, I_BC, I_Q, I_MSE, I_ACT}, {INFO});
    }

    // Adam (+ Polyak for the critic) of one module (0 BC flow, 1 one-step actor, 2 critic) as its own launch on `lane`
    // m2 >= 0: a second module (its nets in net_ids as well) rides in the same launch; m2 == -2: every chunk.
    // Everything the arguments read (the arenas, chunk tables, counters, ticket) is allocated before the first program is built and freed
    // by fql_destroy alone.  The reference is for the sites that append reads or writes (it holds until the next op is pushed).
    Op& adam_for(Program& pr, int m, std::initializer_list<int> net_ids, int lane, int m2 = -1, AdamOpt o = AdamOpt{}) {
        DevState* st = o.st ? o.st : d_state;
            Op a{};
            a.type = OP_ADAM;
            int c0 = mod_chunk0[m], n0 = mod_chunkn[m], c1 = 0, n1 = 0;   // chunk ranges (n0 = -1: all chunks; n1 = 0: no second range)
            a.reads = {st};
            a.writes = {d_partials + mod_chunk0[m] * 4};
            if (m2 >= 0) { c1 = mod_chunk0[m2]; n1 = mod_chunkn[m2]; a.writes.push_back(d_partials + mod_chunk0[m2] * 4); }
            if (m2 == -2) {   // all chunks (the modules' ranges tile [0, n_chunks))
                c0 = 0; n0 = -1;
                for (int mm = 0; mm < 3; ++mm) a.writes.push_back(d_partials + mod_chunk0[mm] * 4);
            }
            AdamArgs aa{P, G, Mu, Nu, P + n_train, d_chunks, st, d_partials, c0, o.polyak >= 0 ? o.polyak : (int)critic_size,
                        o.lr > 0.f ? o.lr : cfg.lr, cfg.tau, -1, n1 > 0 ? n0 : -1, c1};
            if (o.fin) {
                aa.ticket = d_ticket;
                aa.ticket_n = n_chunks;
                aa.fin = fin_args(1);   // (its tl stays -1: the launch's own id is AdamArgs::tl)
            }
            a.k = tl_in(bind(fql_adam_kernel, n0 < 0 ? n_chunks : n0 + n1, aa), offsetof(AdamArgs, tl));
            // the critic's Adam, the first launch of lane 2's tail, also waits for the Euler target the actor-loss kernel behind it reads -
            // one launch with two cross-lane edges instead of two launches with one each (every such edge costs the waiting lane ~10 us)
            if (m == 2 && tgt) a.reads.push_back(tgt);
            for (int mm : {m, m2}) if (visual && mm >= 0) {
                const int m = mm;
                const int ei = m == 2 ? ENC_C : (m == 0 ? ENC_BC : ENC_OS);
                for (const EncStack& st : encs[ei].stacks)
                    for (const ConvL& c : st.conv) {
                        a.reads.push_back(G + c.w); a.reads.push_back(G + c.b);
                        a.writes.push_back(P + c.w);
                        if (m == 2) a.writes.push_back(P + n_train + c.w);
                    }
                const Layer& D = encs[ei].dense;
                a.reads.push_back(G + D.w); a.reads.push_back(G + D.b);
                a.writes.push_back(P + D.w);
                if (m == 2) a.writes.push_back(P + n_train + D.w);
            }
            for (int ni : net_ids)
                for (const Layer& L : nets[ni].layers) {
                    a.reads.push_back(G + L.w); a.reads.push_back(G + L.b);
                    a.writes.push_back(P + L.w);
                    if (L.ln) { a.reads.push_back(G + L.g); a.reads.push_back(G + L.be); a.writes.push_back(P + L.g); }
                    if (ni == NET_C0 || ni == NET_C1) a.writes.push_back(P + n_train + L.w);  // Polyak target
                }
            emit_lane = lane;
            push(pr, a);
            return pr.ops.back();
        }
    // the FQL programs' finalize launch (do_grad_stats: behind an optimizer pass)
    Bound finalize_launch(int do_grad_stats) const {
        return tl_in(bind(fql_finalize_kernel, 1, fin_args(do_grad_stats)), offsetof(FinalizeArgs, tl));
    }

    // The optimizer half of the begin / end pair (data-parallel step: gradients are all-reduced between the halves): per-module Adam
    // as in the fused program - critic and BC flow (gradient bucket 0) + the chain's weight-copy refresh on lane 1, the one-step
    // actor (bucket 1) and the bookkeeping on lane 0.  fql_update_end captures it as one two-lane graph; fql_update_end_split issues
    // lane 1 on the stream that carried bucket 0's all-reduce, so those Adam launches overlap lane 0's tail and bucket 1's reduce.
    // fql_update_end runs it as ONE lane (a captured two-lane graph of five launches pays more for its fork and join than the two Adam launches
    // overlap: the plain data-parallel step at world size 1, collective forced, 2167 -> 2298 updates/s).
    void build_opt_program(Program& pr, bool two_lanes) {
        DevState* st = d_state;
        if (two_lanes) {
            adam_for(pr, 2, {NET_C0, NET_C1}, 1);
            adam_for(pr, 0, {NET_BC}, 1);
            if (use_chain) { emit_lane = 1; emit_wfrag(pr); }
            adam_for(pr, 1, {NET_OS}, 0);
        } else {   // every chunk of every module in ONE Adam launch, then the copies' refresh, then the bookkeeping
            adam_for(pr, 2, {NET_C0, NET_C1, NET_BC, NET_OS}, 0, -2);
            if (use_chain) { emit_lane = 0; emit_wfrag(pr); }
        }
        emit_fin(pr, OP_FINALIZE, finalize_launch(1), offsetof(FinalizeArgs, tl), {&st->info[0], &st->info[4], &st->info[5], &st->info[7], &st->info[9]}, true,
                 {&st->info[10], st});
    }
    // the optimizer program as plain launches on two caller streams (no capture: five launches)
    void run_opt_split(hipStream_t s0, hipStream_t s1) {
        // lane 1 rewrites the critic's and the BC flow's parameters (and the chain's weight copies): it must not pass lane 0's last
        // reader of them, the Euler chain.  After a split begin that point is ev_c; otherwise everything enqueued on s0 so far.
        if (!ev_c) HIP_CHECK(hipEventCreateWithFlags(&ev_c, hipEventDisableTiming));
        if (!split_begun) HIP_CHECK(hipEventRecord(ev_c, s0));
        HIP_CHECK(hipStreamWaitEvent(s1, ev_c, 0));
        split_begun = false;
        const hipStream_t ls[FQL_LANES] = {s0, s1, s1, s1};
        run_launches(prog_opt_split, s0, ls, false);   // s0 ends behind everything of the update
    }

    // fwd + bwd + optimizer in one graph (single-GPU calls): Adam of a module is issued on the lane that produced its
    // gradients as soon as they exist, so 3/4 of the optimizer pass overlaps the tail of the critical lane
    void build_full_program(Program& pr) {
        build_step_program(pr, true);
        DevState* st = d_state;
        // the critic's and the BC flow's Adam as ONE launch (rather than two): both sit at the end of the same lane behind the same
        // dependencies, and every graph node costs the host 3-4 us
        // No finalize launch by default: the two Adam launches below cover every chunk once, each of their workgroups takes a ticket, and the
        // workgroup that takes the last one runs the finalize code (fql_adam_body).  That workgroup may sit in either launch, so the
        // ops keep their own read and write sets and no edge joins the lanes: the ticket, not the schedule, puts the counters'
        // update behind their last reader.  Nothing behind the two launches reads the counters or the infos (the weight-copy
        // refresh does not), and the update ends behind every lane.
        // (the modules' chunk ranges tile [0, n_chunks): were a leaf outside the three trained modules, the ticket would never complete)
        AdamOpt tail;
        tail.fin = fused_tail && mod_chunkn[0] + mod_chunkn[1] + mod_chunkn[2] == n_chunks;
        adam_for(pr, 2, {NET_C0, NET_C1, NET_BC}, fill_lane_full, 0, tail);
        emit_wfrag(pr);   // lane 1, behind the BC flow's Adam: the next update's chain reads the copies
        adam_for(pr, 1, {NET_OS}, 0, -1, tail);
        if (tail.fin) return;
        emit_fin(pr, OP_FINALIZE, finalize_launch(1), offsetof(FinalizeArgs, tl), {&st->info[0], &st->info[4], &st->info[5], &st->info[7], &st->info[9]}, true,
                 {&st->info[10], st});
    }

    // FinalizeArgs of a finalize launch, or of the finalize code inside an Adam launch.  Every field is allocated before the first program is built (build_leaves, create_engine)
    // and freed by fql_destroy alone, so the emit site binds it like any other argument; tl is written at issue time (Bound::tl_at).
    FinalizeArgs fin_args(int do_grad_stats) const {
        return FinalizeArgs{d_state, d_chunks, d_partials, d_leaf_range, n_chunks, n_train_leaves, do_grad_stats, -1};
    }
    // A finalize op (OP_FINALIZE or an agent's *_FIN), on lane 0.  tl_at: where the bound arguments hold FinalizeArgs::tl (-1: the kernel takes none);
    // grad_partials: it also reads the three modules' gradient partials the Adam launch left.
    void emit_fin(Program& pr, OpType type, Bound k, int tl_at, std::vector<const void*> reads, bool grad_partials, std::vector<const void*> writes) {
        k.tl_at = tl_at;
        if (grad_partials) for (int m = 0; m < 3; ++m) reads.push_back(d_partials + mod_chunk0[m] * 4);
        emit_lane = 0;
        emit(pr, type, k, std::move(reads), std::move(writes));
    }
    // the flow-matching loss mean((pred - vel)^2) over B act elements of pass `p` into `info_slot` (IFQL, BC, CFGRL): a payload op, it
    // rides in the side launch of its level
    void emit_loss_bc(Program& pr, const PassBuf& p, const void* info_slot, bool with_grads) {
        const int ad = cfg.act_dim;
        Op op{};
        op.type = OP_LOSS_BC;
        op.lb = LossBcArgs{p.out, vel, with_grads ? p.dz.back() : nullptr, d_state, B, ad, pad16(ad), with_grads ? 1 : 0};
        op.reads = {p.out, vel};
        op.writes = {info_slot};
        if (with_grads) op.writes.push_back(p.dz.back());
        push(pr, op);
    }
    // the tail of every agent's build_*_workspace(): launches and graphs of the programs just built (schedule() reads the ops alone, so
    // no schedule depends on another program's capture); the sources are described again on the next update
    void finish_programs(std::initializer_list<Program*> progs) {
        for (Program* pr : progs) schedule(*pr, ws_allocs);
        for (Program* pr : progs) capture(*pr);
        split_ok = false;
        src_valid = false;
        gsrc_valid = false;
    }

    // ---------------------------------------------------------------------------------------
    // the IFQL update as a program (agents/ifql.py:79-120).  No Euler chain: every level is throughput work on the side lanes.
    //   lane 0: batch assembly; Adam + Polyak over every chunk and the finalize, behind both side lanes
    //   lane 1: value on [obs ; next_obs] (2B rows) -> target pair -> value loss -> value backward (obs half); actor_flow forward, BC loss, backward
    //   lane 2: critic pair forward -> critic loss (waits for value(next_obs) on lane 1) -> critic backward (parameter gradients only)
    // Edges between the forked lanes run 1 -> 2 only (see schedule()).
    // ---------------------------------------------------------------------------------------
    void build_ifql_program(Program& pr, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        DevState* st = d_state;
        const void *I_V = &st->info[IFQL_I_VALUE], *I_C = &st->info[IFQL_I_CRITIC], *I_A = &st->info[IFQL_I_ACTOR];
        wide_tiles = true;
        allow64 = true;
        emit_lane = 0;
        {
            const IfqlPrepArgs iprep{d_src, st, seed, B, od, ad, nets[NET_OS].in_p(), nets[NET_C0].in_p(), nets[NET_BC].in_p(), ap,
                                     X_v, X_c1, X_bc, vel, w_rew, w_mask};
            emit(pr, OP_IFQL_PREP, bind(fql_ifql_prep_kernel, (iprep.B + 3) / 4, iprep), {}, {X_v, X_c1, X_bc, vel, w_rew, w_mask});
        }
        emit_lane = 1;
        emit_forward(pr, p_v, with_grads);                        // value(obs) ifql.py:34, value(next_obs) ifql.py:47
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_ct[e], false);   // target_critic(obs, actions) ifql.py:33
        {
            const IfqlValueArgs iv{p_v.out, p_ct[0].out, p_ct[1].out, with_grads ? p_v.dz.back() : nullptr, st, B, expectile};
            Op& op = emit(pr, OP_IFQL_LOSS_V, bind(fql_ifql_loss_value_kernel, 1, iv), {p_v.out, p_ct[0].out, p_ct[1].out}, {I_V});
            if (with_grads) op.writes.push_back(p_v.dz.back());
        }
        if (with_grads) emit_backward(pr, p_v, 0, B, true, false);
        emit_forward(pr, p_bc, with_grads);                       // actor_flow(obs, x_t, t) ifql.py:71
        emit_loss_bc(pr, p_bc, I_A, with_grads);
        if (with_grads) emit_backward(pr, p_bc, 0, B, true, false);
        emit_lane = 2;
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_c1[e], with_grads);   // critic(obs, actions) ifql.py:50
        {
            const IfqlCriticArgs ic{p_v.out + (size_t)B * nets[NET_OS].layers.back().out_p, p_c1[0].out, p_c1[1].out, w_rew, w_mask,
                                    with_grads ? p_c1[0].dz.back() : nullptr, with_grads ? p_c1[1].dz.back() : nullptr, st, B, cfg.discount};
            Op& op = emit(pr, OP_IFQL_LOSS_C, bind(fql_ifql_loss_critic_kernel, 1, ic), {p_v.out, p_c1[0].out, p_c1[1].out, w_rew, w_mask}, {I_C});
            if (with_grads) { op.writes.push_back(p_c1[0].dz.back()); op.writes.push_back(p_c1[1].dz.back()); }
        }
        if (with_grads)
            for (int e = 0; e < 2; ++e) emit_backward(pr, p_c1[e], 0, B, true, false);
        if (with_grads) adam_for(pr, 2, {NET_C0, NET_C1, NET_BC, NET_OS}, 0, -2);   // every chunk, one launch; Polyak from the pre-step critic
        emit_fin(pr, OP_IFQL_FIN, bind(fql_ifql_finalize_kernel, 1, fin_args(with_grads ? 1 : 0)), offsetof(FinalizeArgs, tl), {I_V, I_C, I_A},
                 with_grads, {&st->info[8], st});
    }

    void build_ifql_workspace() {
        const int ap = pad16(cfg.act_dim);
        auto& W = ws_allocs;
        X_v = dalloc(W, (size_t)2 * B * nets[NET_OS].in_p());
        X_c1 = dalloc(W, (size_t)B * nets[NET_C0].in_p());
        X_bc = dalloc(W, (size_t)B * nets[NET_BC].in_p());
        vel = dalloc(W, (size_t)B * ap);
        w_rew = dalloc(W, B); w_mask = dalloc(W, B);
        p_v = make_pass(W, NET_OS, 2 * B, X_v, true, false);
        p_bc = make_pass(W, NET_BC, B, X_bc, true, false);
        for (int e = 0; e < 2; ++e) {
            p_c1[e] = make_pass(W, NET_C0 + e, B, X_c1, true, false);
            p_ct[e] = make_pass(W, NET_T0 + e, B, X_c1, false, false);
        }
        build_ifql_program(prog_full, true);
        build_ifql_program(prog_loss, false);
        finish_programs({&prog_full, &prog_loss});
    }

    // ---------------------------------------------------------------------------------------
    // the ReBRAC update as a program (agents/rebrac.py:86-134).  No Euler chain: throughput work on the side lanes.
    //   lane 0: batch assembly; Adam over every chunk (+ Polyak of critic and actor on a full step) and the finalize, behind both side lanes
    //   lane 1: target actor -> target action -> target critic pair; full steps: actor -> critic pair on [obs | a] -> actor loss ->
    //           the pair's input gradient -> dL/dmean -> actor backward
    //   lane 2: critic pair forward -> critic loss (waits for the target pair on lane 1) -> critic backward (parameter gradients only)
    // Edges between the forked lanes run 1 -> 2 only (see schedule()).  with_grads = false: the loss probe (no backward, no finalize).
    // ---------------------------------------------------------------------------------------
    void build_rebrac_program(Program& pr, bool full_update, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        const int inp_a = nets[NET_BC].in_p(), inp_c = nets[NET_C0].in_p();
        DevState* st = d_state;
        const void *I_C = &st->info[REBRAC_I_CRITIC], *I_A = &st->info[REBRAC_I_ACTOR];
        const bool zero_actor = with_grads && !full_update;
        const Net& na = nets[NET_BC];
        wide_tiles = true;
        allow64 = true;
        emit_lane = 0;
        {
            const RebracPrepArgs rprep{d_src, st, seed, B, od, ad, inp_a, inp_c, ap, X_c1, X_t, X_q, X_a, X_ta, w_act, w_nact, w_noise,
                                       w_rew, w_mask, zero_actor ? G + na.off : nullptr, zero_actor ? (int64_t)na.size : 0};
            Op& op = emit(pr, OP_REBRAC_PREP, bind(fql_rebrac_prep_kernel, (rprep.B + 3) / 4, rprep), {},
                          {X_c1, X_t, X_q, X_a, X_ta, w_act, w_nact, w_noise, w_rew, w_mask});
            if (zero_actor)   // critic-only step: the actor's gradient is zero (rebrac.py:104-106), not the last full step's
                for (const Layer& L : na.layers) {
                    op.writes.push_back(G + L.w); op.writes.push_back(G + L.b);
                    if (L.ln) { op.writes.push_back(G + L.g); op.writes.push_back(G + L.be); }
                }
        }
        auto act_op = [&](const PassBuf& p, const float* noise, float* X, bool target) {
            const RebracActArgs ract{p.out, noise, X, 0, 0, B, ad, ap, ap, inp_c, od, 0, target ? 1 : 0, rcfg.tanh_squash, target ? 1 : 0,
                                     rcfg.actor_noise, rcfg.actor_noise_clip};
            Op& op = emit(pr, OP_REBRAC_ACT, bind(fql_rebrac_act_kernel, (ract.n * ract.ad + FQL_THREADS - 1) / FQL_THREADS, ract), {p.out}, {X});
            if (noise) op.reads.push_back(noise);
        };
        emit_lane = 1;
        emit_forward(pr, p_ta, false);                                  // target_actor(next_obs)  rebrac.py:28
        act_op(p_ta, w_noise, X_t, true);                               // a' = clip(mode + clip(noise), -1, 1)  rebrac.py:29-34
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_ct[e], false);   // target_critic(next_obs, a')  rebrac.py:36
        if (full_update) {
            emit_forward(pr, p_a, with_grads);                          // actor(obs)  rebrac.py:57
            act_op(p_a, nullptr, X_q, false);                           // a = mode  rebrac.py:58
            for (int e = 0; e < 2; ++e) emit_forward(pr, p_q[e], with_grads);   // critic(obs, a), stored params  rebrac.py:61
            {
                const RebracActorArgs ra{p_q[0].out, p_q[1].out, X_q, w_act, with_grads ? p_q[0].dz.back() : nullptr,
                                         with_grads ? p_q[1].dz.back() : nullptr, st, B, od, ad, inp_c, ap, rcfg.alpha_actor};
                Op& op = emit(pr, OP_REBRAC_LOSS_A, bind(fql_rebrac_loss_actor_kernel, 1, ra), {p_q[0].out, p_q[1].out, X_q, w_act}, {I_A});
                if (with_grads) { op.writes.push_back(p_q[0].dz.back()); op.writes.push_back(p_q[1].dz.back()); }
            }
            if (with_grads) {
                for (int e = 0; e < 2; ++e) emit_backward(pr, p_q[e], 0, B, false, true);   // dQ/da only: the critic's params get no gradient
                const RebracActorGradArgs rag{p_q[0].dx0, p_q[1].dx0, X_q, w_act, p_a.dz.back(), B, od, ad, inp_c, ap,
                                              rcfg.alpha_actor * 2.0f / (float)B, rcfg.tanh_squash};
                emit(pr, OP_REBRAC_AGRAD, bind(fql_rebrac_actor_grad_kernel, (rag.B * rag.ad + FQL_THREADS - 1) / FQL_THREADS, rag),
                     {p_q[0].dx0, p_q[1].dx0, X_q, w_act}, {p_a.dz.back()});
                emit_backward(pr, p_a, 0, B, true, false);
            }
        }
        emit_lane = 2;
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_c1[e], with_grads);   // critic(obs, actions)  rebrac.py:44
        {
            const RebracCriticArgs rc{p_c1[0].out, p_c1[1].out, p_ct[0].out, p_ct[1].out, X_t, w_nact, w_rew, w_mask,
                                      with_grads ? p_c1[0].dz.back() : nullptr, with_grads ? p_c1[1].dz.back() : nullptr, st, B, od, ad, inp_c, ap,
                                      cfg.discount, rcfg.alpha_critic};
            Op& op = emit(pr, OP_REBRAC_LOSS_C, bind(fql_rebrac_loss_critic_kernel, 1, rc),
                          {p_c1[0].out, p_c1[1].out, p_ct[0].out, p_ct[1].out, X_t, w_nact, w_rew, w_mask}, {I_C});
            if (with_grads) { op.writes.push_back(p_c1[0].dz.back()); op.writes.push_back(p_c1[1].dz.back()); }
        }
        if (!with_grads) return;
        for (int e = 0; e < 2; ++e) emit_backward(pr, p_c1[e], 0, B, true, false);
        // every chunk in one launch (the actor's too: on a critic-only step Adam still moves it with a zero gradient); Polyak from the
        // pre-step critic and actor on full steps only (rebrac.py:112-120,131-133)
        AdamOpt ao;
        if (!full_update) ao.polyak = 0;
        Op& a = adam_for(pr, 0, {NET_C0, NET_C1, NET_BC}, 0, -2, ao);
        if (full_update) for (const Layer& L : na.layers) a.writes.push_back(P + n_train + L.w);   // the target actor
        emit_fin(pr, OP_REBRAC_FIN, bind(fql_rebrac_finalize_kernel, 1, fin_args(1), full_update ? 1 : 0), offsetof(FinalizeArgs, tl), {I_C, I_A},
                 true, {&st->info[8], st});
    }

    void build_rebrac_workspace() {
        const int ap = pad16(cfg.act_dim);
        const int inp_a = nets[NET_BC].in_p(), inp_c = nets[NET_C0].in_p();
        auto& W = ws_allocs;
        in_nact = dalloc(W, (size_t)B * cfg.act_dim);   // staging of a host batch's next_actions
        X_c1 = dalloc(W, (size_t)B * inp_c); X_t = dalloc(W, (size_t)B * inp_c); X_q = dalloc(W, (size_t)B * inp_c);
        X_a = dalloc(W, (size_t)B * inp_a); X_ta = dalloc(W, (size_t)B * inp_a);
        w_act = dalloc(W, (size_t)B * ap); w_nact = dalloc(W, (size_t)B * ap); w_noise = dalloc(W, (size_t)B * ap);
        w_rew = dalloc(W, B); w_mask = dalloc(W, B);
        p_a = make_pass(W, NET_BC, B, X_a, true, false);
        p_ta = make_pass(W, NET_TA, B, X_ta, false, false);
        for (int e = 0; e < 2; ++e) {
            p_c1[e] = make_pass(W, NET_C0 + e, B, X_c1, true, false);
            p_ct[e] = make_pass(W, NET_T0 + e, B, X_t, false, false);
            p_q[e] = make_pass(W, NET_C0 + e, B, X_q, true, true);
        }
        build_rebrac_program(prog_full, true, true);
        build_rebrac_program(prog_critic, false, true);
        build_rebrac_program(prog_loss, true, false);
        finish_programs({&prog_full, &prog_critic, &prog_loss});
    }
    // ---------------------------------------------------------------------------------------
    // the SAC update as a program (agents/sac.py:23-122).  No Euler chain: throughput work on the side lanes.
    //   lane 0: batch assembly (+ eps_c, eps_n); Adam over every chunk (Polyak of the critic) and the finalize, behind both side lanes
    //   lane 1: actor over [obs ; next_obs] -> sample + log-prob (a' into the target pair's input, a into [obs | a]) -> critic pair on
    //           [obs | a] -> actor / temperature loss -> the pair's input gradient -> dL/d(heads) -> actor backward (obs rows)
    //   lane 2: critic pair forward -> target pair forward (waits for a' on lane 1) -> critic loss -> critic backward (parameter gradients)
    // Edges between the forked lanes run 1 -> 2 only (see schedule()).  with_grads = false: the loss probe (no backward, no finalize).
    // ---------------------------------------------------------------------------------------
    void build_sac_program(Program& pr, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        const int inp_a = nets[NET_BC].in_p(), inp_c = nets[NET_C0].in_p();
        DevState* st = d_state;
        const void *I_C = &st->info[SAC_I_CRITIC], *I_A = &st->info[SAC_I_ACTOR], *I_Q = &st->info[SAC_I_Q];
        const float* la = P + alpha_off;
        wide_tiles = true;
        allow64 = true;
        emit_lane = 0;
        {
            const SacPrepArgs sprep{d_src, st, seed, B, od, ad, inp_a, inp_c, ap, X_c1, X_t, X_q, X_a, w_eps, w_rew, w_mask};
            emit(pr, OP_SAC_PREP, bind(fql_sac_prep_kernel, (sprep.B + 3) / 4, sprep), {}, {X_c1, X_t, X_q, X_a, w_eps, w_rew, w_mask});
        }
        emit_lane = 1;
        emit_forward(pr, p_a, with_grads);   // actor(obs), actor(next_obs)  sac.py:26,61
        {   // a, lp (obs rows) and a', lp' (next rows)  sac.py:27,62
            const SacActArgs sact{p_a.out, w_eps, X_q, X_t, lp_buf, 0, 0, 2 * B, ad, ap, ap, inp_c, od, 0, B, 1, scfg.tanh_squash, 0, 1.0f};
            emit(pr, OP_SAC_ACT, bind(fql_sac_act_kernel, (sact.n + FQL_THREADS - 1) / FQL_THREADS, sact), {p_a.out, w_eps}, {X_q, X_t, lp_buf});
        }
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_q[e], with_grads);   // critic(obs, a), stored params  sac.py:65
        {
            const SacActorArgs sa{p_q[0].out, p_q[1].out, lp_buf, p_a.out, la, with_grads ? G + alpha_off : nullptr,
                                  with_grads ? p_q[0].dz.back() : nullptr, with_grads ? p_q[1].dz.back() : nullptr, st, B, ad, ap, target_entropy};
            Op& op = emit(pr, OP_SAC_LOSS_A, bind(fql_sac_loss_actor_kernel, 1, sa), {p_q[0].out, p_q[1].out, lp_buf, p_a.out, la}, {I_A, I_Q});
            if (with_grads) { op.writes.push_back(G + alpha_off); op.writes.push_back(p_q[0].dz.back()); op.writes.push_back(p_q[1].dz.back()); }
        }
        if (with_grads) {
            for (int e = 0; e < 2; ++e) emit_backward(pr, p_q[e], 0, B, false, true);   // dQ/da only: the critic's params get no gradient
            const SacActorGradArgs sag{p_q[0].dx0, p_q[1].dx0, X_q, p_a.out, w_eps, la, p_a.dz.back(), B, od, ad, inp_c, ap, scfg.tanh_squash};
            emit(pr, OP_SAC_AGRAD, bind(fql_sac_actor_grad_kernel, (sag.B * sag.ad + FQL_THREADS - 1) / FQL_THREADS, sag),
                 {p_q[0].dx0, p_q[1].dx0, X_q, p_a.out, w_eps, la}, {p_a.dz.back()});
            emit_backward(pr, p_a, 0, B, true, false);
        }
        emit_lane = 2;
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_c1[e], with_grads);   // critic(obs, actions)  sac.py:46
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_ct[e], false);         // target_critic(next_obs, a')  sac.py:30
        {
            const SacCriticArgs sc{p_c1[0].out, p_c1[1].out, p_ct[0].out, p_ct[1].out, lp_buf + B, w_rew, w_mask, la,
                                   with_grads ? p_c1[0].dz.back() : nullptr, with_grads ? p_c1[1].dz.back() : nullptr, st, B,
                                   cfg.q_agg == 1 ? 1 : 0, scfg.backup_entropy ? 1 : 0, cfg.discount};
            Op& op = emit(pr, OP_SAC_LOSS_C, bind(fql_sac_loss_critic_kernel, 1, sc),
                          {p_c1[0].out, p_c1[1].out, p_ct[0].out, p_ct[1].out, lp_buf, w_rew, w_mask, la}, {I_C});
            if (with_grads) { op.writes.push_back(p_c1[0].dz.back()); op.writes.push_back(p_c1[1].dz.back()); }
        }
        if (!with_grads) return;
        for (int e = 0; e < 2; ++e) emit_backward(pr, p_c1[e], 0, B, true, false);
        // every chunk in one launch (log_value's too); Polyak of the target critic from the pre-step critic (sac.py:113)
        adam_for(pr, 0, {NET_C0, NET_C1, NET_BC}, 0, -2);
        Op& a = pr.ops.back();
        a.reads.push_back(G + alpha_off);
        a.writes.push_back(P + alpha_off);
        emit_fin(pr, OP_SAC_FIN, bind(fql_sac_finalize_kernel, 1, fin_args(1)), offsetof(FinalizeArgs, tl), {I_C, I_A, I_Q}, true, {&st->info[10], st});
    }

    void build_sac_workspace() {
        const int ap = pad16(cfg.act_dim);
        const int inp_a = nets[NET_BC].in_p(), inp_c = nets[NET_C0].in_p();
        auto& W = ws_allocs;
        X_c1 = dalloc(W, (size_t)B * inp_c); X_t = dalloc(W, (size_t)B * inp_c); X_q = dalloc(W, (size_t)B * inp_c);
        X_a = dalloc(W, (size_t)2 * B * inp_a);
        w_eps = dalloc(W, (size_t)2 * B * ap); lp_buf = dalloc(W, (size_t)2 * B);
        w_rew = dalloc(W, B); w_mask = dalloc(W, B);
        p_a = make_pass(W, NET_BC, 2 * B, X_a, true, false);
        for (int e = 0; e < 2; ++e) {
            p_c1[e] = make_pass(W, NET_C0 + e, B, X_c1, true, false);
            p_ct[e] = make_pass(W, NET_T0 + e, B, X_t, false, false);
            p_q[e] = make_pass(W, NET_C0 + e, B, X_q, true, true);
        }
        build_sac_program(prog_full, true);
        build_sac_program(prog_loss, false);
        finish_programs({&prog_full, &prog_loss});
    }
    // ---------------------------------------------------------------------------------------
    // the BC update as a program (agents/bc.py:48-84): ONE lane, no cross-lane edge.  Batch assembly -> policy forward (64-column LDS
    // tiles where the shapes allow, LayerNorm on the A tile) -> flow-matching loss (rides in the side launch of its level) -> backward
    // (weight gradients and LayerNorm backward share the dgrad launches) -> Adam over every chunk -> finalize.
    // with_grads = false: the loss probe (forward and loss only: it writes info slot 5, none of the four slots fql_read_info_n reads).
    // ---------------------------------------------------------------------------------------
    void build_bc_program(Program& pr, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        DevState* st = d_state;
        const void* I_L = &st->info[BC_I_LOSS];
        wide_tiles = true;
        allow64 = true;
        lane0_64 = true;
        emit_lane = 0;
        {
            const BcPrepArgs bprep{d_src, st, seed, d_emb, B, od, ad, nets[NET_BC].in_p(), ap, bc_steps, X_bc, vel};
            emit(pr, OP_BC_PREP, bind(fql_bc_prep_kernel, (bprep.B + 3) / 4, bprep), {}, {X_bc, vel});
        }
        emit_forward(pr, p_bc, with_grads);        // policy(obs, x_t, t)  bc.py:67
        emit_loss_bc(pr, p_bc, I_L, with_grads);   // mean((vel - pred)^2) over B act elements  bc.py:69
        if (with_grads) {
            emit_backward(pr, p_bc, 0, B, true, false);
            adam_for(pr, 0, {NET_BC}, 0, -2);   // every chunk in one launch; critic_size = 0: no Polyak range
            emit_fin(pr, OP_BC_FIN, bind(fql_bc_finalize_kernel, 1, fin_args(1)), offsetof(FinalizeArgs, tl), {I_L, d_partials}, false,
                     {&st->info[0], &st->info[10], st});
        }
        lane0_64 = false;
    }
    void build_bc_workspace() {
        const int ap = pad16(cfg.act_dim);
        auto& W = ws_allocs;
        X_bc = dalloc(W, (size_t)B * nets[NET_BC].in_p());
        vel = dalloc(W, (size_t)B * ap);
        p_bc = make_pass(W, NET_BC, B, X_bc, true, false);
        build_bc_program(prog_full, true);
        build_bc_program(prog_loss, false);
        finish_programs({&prog_full, &prog_loss});
    }
    // ---------------------------------------------------------------------------------------
    // the CFGRL update as a program (agents/cfgrl.py:22-68): BC's single lane with a goal block in the input rows.  Batch assembly (index,
    // goal and mask draw, gather, the goal columns of a dropped row from the CURRENT unc_embed leaf) -> actor_flow forward -> flow-matching
    // loss -> backward (no input-gradient pass) -> the embedding gradient from dZ0 of the dropped rows -> Adam over every chunk -> finalize.
    // with_grads = false: the loss probe (it writes info slot 5 and the probe half of the row read-back only).
    // ---------------------------------------------------------------------------------------
    void build_cfgrl_program(Program& pr, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad), Gd = gcfg.goal_dim;
        DevState* st = d_state;
        const void* I_L = &st->info[CFGRL_I_LOSS];
        const int half = with_grads ? 0 : 1;
        unsigned char* mask = cf_mask + (size_t)half * B;
        int64_t* rows = cf_rows + (size_t)half * 2 * B;
        uint32_t* draws = cf_draws + (size_t)half * CFGRL_NUM_DRAWS * B;
        const Layer& l0 = nets[NET_BC].layers[0];
        wide_tiles = true;
        allow64 = true;
        lane0_64 = true;
        emit_lane = 0;
        {
            const CfgrlPrepArgs gp{d_src, d_gsrc, st, seed, P + emb_off, B, od, Gd, ad, nets[NET_BC].in_p(), ap, X_bc, vel, rows, draws, mask};
            emit(pr, OP_CFGRL_PREP, bind(fql_cfgrl_prep_kernel, (gp.B + 3) / 4, gp), {P + emb_off}, {X_bc, vel, mask, rows, draws});
        }
        emit_forward(pr, p_bc, with_grads);        // actor_flow(obs, x_t, t, goals)  cfgrl.py:37
        emit_loss_bc(pr, p_bc, I_L, with_grads);   // mean((pred - vel)^2) over B act elements  cfgrl.py:38
        if (with_grads) {
            emit_backward(pr, p_bc, 0, B, true, false);
            const CfgrlEmbedGradArgs eg{p_bc.dz[0], P + l0.w + (size_t)od * l0.out_p, mask, G + emb_off, B, l0.out_p, Gd};
            emit(pr, OP_CFGRL_EGRAD, bind(fql_cfgrl_embed_grad_kernel, 1, eg), {p_bc.dz[0], P + l0.w, mask}, {G + emb_off});
            adam_for(pr, 0, {NET_BC}, 0, -2);   // every chunk in one launch; critic_size = 0: no Polyak range
            Op& a = pr.ops.back();
            a.reads.push_back(G + emb_off);
            a.writes.push_back(P + emb_off);
            emit_fin(pr, OP_CFGRL_FIN, bind(fql_cfgrl_finalize_kernel, 1, fin_args(1)), offsetof(FinalizeArgs, tl), {I_L, d_partials}, false,
                     {&st->info[0], &st->info[10], st});
        }
        lane0_64 = false;
    }
    void build_cfgrl_workspace() {
        const int ap = pad16(cfg.act_dim), Gd = gcfg.goal_dim;
        auto& W = ws_allocs;
        X_bc = dalloc(W, (size_t)B * nets[NET_BC].in_p());
        vel = dalloc(W, (size_t)B * ap);
        in_goal = dalloc(W, (size_t)B * Gd);
        in_cfg = (unsigned char*)dalloc(W, (size_t)(B + 3) / 4);
        cf_mask = (unsigned char*)dalloc(W, (size_t)(2 * B + 3) / 4);
        cf_rows = (int64_t*)dalloc(W, (size_t)2 * 2 * B * 2);
        cf_draws = (uint32_t*)dalloc(W, (size_t)2 * CFGRL_NUM_DRAWS * B);
        p_bc = make_pass(W, NET_BC, B, X_bc, true, false);
        build_cfgrl_program(prog_full, true);
        build_cfgrl_program(prog_loss, false);
        finish_programs({&prog_full, &prog_loss});
    }

    // multiply-accumulates per row of a net's forward, algorithmic (full GEMM shapes at the logical widths), and of its first layer alone
    // (a backward pass without the input gradient costs 2 net_macs - first_macs)
    static int64_t net_macs(const Net& n) { int64_t m = 0; for (const Layer& L : n.layers) m += (int64_t)L.in * L.out; return m; }
    static int64_t first_macs(const Net& n) { return (int64_t)n.layers[0].in * n.layers[0].out; }

    // multiply-accumulates of one BC update per batch row, algorithmic: forward + backward without the input gradient
    int64_t bc_macs() const { return (3 * net_macs(nets[NET_BC]) - first_macs(nets[NET_BC])) * (int64_t)B; }

    // multiply-accumulates of one SAC update per batch row, algorithmic (the heads are H x 2 act, not the padded 2 ap of the stored layer)
    int64_t sac_macs() const {
        const Layer& heads = nets[NET_BC].layers.back();
        const int64_t ac = net_macs(nets[NET_BC]) - (int64_t)heads.in * (heads.out - 2 * cfg.act_dim), cr = net_macs(nets[NET_C0]);
        // actor on 2B rows; target pair; critic pair forward + backward without the input gradient
        int64_t m = 2 * ac + 2 * cr + 2 * cr + 2 * (2 * cr - first_macs(nets[NET_C0]));
        // the pair on [obs | a] forward + input gradient; actor backward on the obs rows without the input gradient
        m += 2 * cr + 2 * cr + (2 * ac - first_macs(nets[NET_BC]));
        return m * (int64_t)B;
    }

    // ---------------------------------------------------------------------------------------
    // the IQL update as a program (agents/iql.py:28-156).  No Euler chain: throughput work on the side lanes.
    //   lane 0: batch assembly (+ eps); Adam + Polyak over every chunk and the finalize, behind both side lanes
    //   lane 1: value on [obs ; next_obs] (2B rows) -> target pair -> value loss -> value backward (obs half); actor forward -> Gaussian head
    //           (log_prob, squared error; ddpgbc: q_actions into [obs | .]); ddpgbc: critic pair on [obs | q_actions] -> actor loss
    //   lane 2: critic pair forward -> critic loss (waits for value(next_obs) on lane 1) -> critic backward (parameter gradients only);
    //           awr: the actor loss on the q1, q2 and v those forward passes left (no second pass); ddpgbc: the pair's input gradient ->
    //           head gradient; then the actor's backward
    // Edges between the forked lanes run 1 -> 2 only (see schedule()).  with_grads = false: the loss probe (no backward; its finalize
    // writes the probe half of iql_info).
    // ---------------------------------------------------------------------------------------
    void build_iql_program(Program& pr, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        const int inp_v = nets[NET_OS].in_p(), inp_c = nets[NET_C0].in_p(), inp_a = nets[NET_BC].in_p();
        const bool ddpg = qcfg.actor_loss == 1, has_ls = !qcfg.const_std;
        DevState* st = d_state;
        const void *I_V = &st->info[IFQL_I_VALUE], *I_C = &st->info[IFQL_I_CRITIC];
        float* out = iql_info + (with_grads ? 0 : IQL_INFO_STRIDE);
        const void* I_A = out + IQL_I_ACTOR;
        const float* ls = has_ls ? P + ls_off : nullptr;
        float* g_ls = has_ls && with_grads ? G + ls_off : nullptr;
        float* eps = ddpg && has_ls ? w_eps : nullptr;
        wide_tiles = true;
        allow64 = true;
        emit_lane = 0;
        {
            const IqlPrepArgs qprep{d_src, st, seed, B, od, ad, inp_v, inp_c, inp_a, ap, X_v, X_c1, X_a, X_q, w_act, eps, w_rew, w_mask};
            Op& op = emit(pr, OP_IQL_PREP, bind(fql_iql_prep_kernel, (qprep.B + 3) / 4, qprep), {}, {X_v, X_c1, X_a, w_act, w_rew, w_mask});
            if (X_q) op.writes.push_back(X_q);
            if (eps) op.writes.push_back(eps);
        }
        emit_lane = 1;
        emit_forward(pr, p_v, with_grads);                              // value(obs) iql.py:32, value(next_obs) iql.py:44
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_ct[e], false);   // target_critic(obs, actions) iql.py:30
        {
            const IfqlValueArgs iv{p_v.out, p_ct[0].out, p_ct[1].out, with_grads ? p_v.dz.back() : nullptr, st, B, qcfg.expectile};
            Op& op = emit(pr, OP_IFQL_LOSS_V, bind(fql_ifql_loss_value_kernel, 1, iv), {p_v.out, p_ct[0].out, p_ct[1].out}, {I_V});
            if (with_grads) op.writes.push_back(p_v.dz.back());
        }
        if (with_grads) emit_backward(pr, p_v, 0, B, true, false);
        emit_forward(pr, p_a, with_grads);                              // actor(obs) iql.py:69,85
        {   // log_prob(actions) iql.py:70,95; q_actions iql.py:86-89
            const IqlHeadArgs qhead{p_a.out, ls, w_act, eps, lp_buf, se_buf, ddpg ? X_q : nullptr, B, od, ad, ap, inp_c};
            Op& op = emit(pr, OP_IQL_HEAD, bind(fql_iql_head_kernel, (qhead.B + FQL_THREADS - 1) / FQL_THREADS, qhead), {p_a.out, w_act},
                          {lp_buf, se_buf});
            if (ls) op.reads.push_back(ls);
            if (eps) op.reads.push_back(eps);
            if (ddpg) op.writes.push_back(X_q);
        }
        if (ddpg) {
            for (int e = 0; e < 2; ++e) emit_forward(pr, p_q[e], with_grads);   // critic(obs, q_actions), stored params  iql.py:90
            const IqlDdpgArgs qddpg{p_q[0].out, p_q[1].out, lp_buf, se_buf, ls, with_grads ? p_q[0].dz.back() : nullptr,
                                    with_grads ? p_q[1].dz.back() : nullptr, out, B, ad, qcfg.alpha};
            Op& op = emit(pr, OP_IQL_LOSS_DDPGBC, bind(fql_iql_loss_ddpgbc_kernel, 1, qddpg), {p_q[0].out, p_q[1].out, lp_buf, se_buf}, {I_A});
            if (ls) op.reads.push_back(ls);
            if (with_grads) { op.writes.push_back(p_q[0].dz.back()); op.writes.push_back(p_q[1].dz.back()); }
        }
        emit_lane = 2;
        for (int e = 0; e < 2; ++e) emit_forward(pr, p_c1[e], with_grads);   // critic(obs, actions) iql.py:47 (and :62: the same numbers)
        {
            const IfqlCriticArgs ic{p_v.out + (size_t)B * nets[NET_OS].layers.back().out_p, p_c1[0].out, p_c1[1].out, w_rew, w_mask,
                                    with_grads ? p_c1[0].dz.back() : nullptr, with_grads ? p_c1[1].dz.back() : nullptr, st, B, cfg.discount};
            Op& op = emit(pr, OP_IFQL_LOSS_C, bind(fql_ifql_loss_critic_kernel, 1, ic), {p_v.out, p_c1[0].out, p_c1[1].out, w_rew, w_mask}, {I_C});
            if (with_grads) { op.writes.push_back(p_c1[0].dz.back()); op.writes.push_back(p_c1[1].dz.back()); }
        }
        if (with_grads)
            for (int e = 0; e < 2; ++e) emit_backward(pr, p_c1[e], 0, B, true, false);
        if (!ddpg) {
            const IqlAwrArgs qawr{p_c1[0].out, p_c1[1].out, p_v.out, lp_buf, se_buf, p_a.out, w_act, ls, with_grads ? p_a.dz.back() : nullptr,
                                  ls_part, g_ls, out, B, ad, ap, qcfg.alpha};
            Op& op = emit(pr, OP_IQL_LOSS_AWR, bind(fql_iql_loss_awr_kernel, 1, qawr),
                          {p_c1[0].out, p_c1[1].out, p_v.out, lp_buf, se_buf, p_a.out, w_act}, {I_A});
            if (ls) op.reads.push_back(ls);
            if (with_grads) op.writes.push_back(p_a.dz.back());
            if (g_ls) { op.writes.push_back(ls_part); op.writes.push_back(g_ls); }
        } else if (with_grads) {
            for (int e = 0; e < 2; ++e) emit_backward(pr, p_q[e], 0, B, false, true);   // dQ/da only: the critic's params get no gradient here
            const IqlActorGradArgs qag{p_q[0].dx0, p_q[1].dx0, p_a.out, w_act, eps, ls, p_a.dz.back(), ls_part, g_ls, B, od, ad, ap, inp_c, qcfg.alpha};
            Op& op = emit(pr, OP_IQL_AGRAD, bind(fql_iql_actor_grad_kernel, 1, qag), {p_q[0].dx0, p_q[1].dx0, p_a.out, w_act}, {p_a.dz.back()});
            if (ls) op.reads.push_back(ls);
            if (eps) op.reads.push_back(eps);
            if (g_ls) { op.writes.push_back(ls_part); op.writes.push_back(g_ls); }
        }
        if (with_grads) {
            emit_backward(pr, p_a, 0, B, true, false);
            adam_for(pr, 2, {NET_C0, NET_C1, NET_BC, NET_OS}, 0, -2);   // every chunk, one launch; Polyak from the pre-step critic (iql.py:154)
            if (has_ls) {
                Op& a = pr.ops.back();
                a.reads.push_back(G + ls_off);
                a.writes.push_back(P + ls_off);
            }
        }
        emit_fin(pr, OP_IQL_FIN, bind(fql_iql_finalize_kernel, 1, IqlFinalizeArgs{fin_args(with_grads ? 1 : 0), out, ddpg ? IQL_N_DDPGBC : IQL_N_AWR}),
                 offsetof(IqlFinalizeArgs, fin.tl), {I_V, I_C, I_A}, with_grads, {out, st});
    }

    void build_iql_workspace() {
        const int ap = pad16(cfg.act_dim);
        const int inp_c = nets[NET_C0].in_p();
        const bool ddpg = qcfg.actor_loss == 1;
        auto& W = ws_allocs;
        X_v = dalloc(W, (size_t)2 * B * nets[NET_OS].in_p());
        X_c1 = dalloc(W, (size_t)B * inp_c);
        X_a = dalloc(W, (size_t)B * nets[NET_BC].in_p());
        X_q = ddpg ? dalloc(W, (size_t)B * inp_c) : nullptr;
        w_act = dalloc(W, (size_t)B * ap); w_eps = dalloc(W, (size_t)B * ap); ls_part = dalloc(W, (size_t)B * ap);
        lp_buf = dalloc(W, B); se_buf = dalloc(W, B);
        w_rew = dalloc(W, B); w_mask = dalloc(W, B);
        p_v = make_pass(W, NET_OS, 2 * B, X_v, true, false);
        p_a = make_pass(W, NET_BC, B, X_a, true, false);
        for (int e = 0; e < 2; ++e) {
            p_c1[e] = make_pass(W, NET_C0 + e, B, X_c1, true, false);
            p_ct[e] = make_pass(W, NET_T0 + e, B, X_c1, false, false);
            if (ddpg) p_q[e] = make_pass(W, NET_C0 + e, B, X_q, true, true);
        }
        build_iql_program(prog_full, true);
        build_iql_program(prog_loss, false);
        finish_programs({&prog_full, &prog_loss});
    }
    // multiply-accumulates of one IQL update per batch row, algorithmic (full GEMM shapes at the logical widths)
    int64_t iql_macs() const {
        const int64_t va = net_macs(nets[NET_OS]), ac = net_macs(nets[NET_BC]), cr = net_macs(nets[NET_C0]);
        // value on 2B rows + its backward on B; target pair; critic pair forward + backward (no input gradient); actor forward + backward
        int64_t m = 2 * va + (2 * va - first_macs(nets[NET_OS])) + 2 * cr + 2 * cr + 2 * (2 * cr - first_macs(nets[NET_C0])) + ac + (2 * ac - first_macs(nets[NET_BC]));
        if (qcfg.actor_loss == 1) m += 2 * cr + 2 * cr;   // ddpgbc: the pair on [obs | q_actions] forward + input gradient
        return m * (int64_t)B;
    }


    // ---------------------------------------------------------------------------------------
    // the IQL-diffusion update as a program (agents/iql_diffusion.py:94-247), one per step kind: (update_critic, update_actor) in
    // {(1, 1), (1, 0), (0, 1), (0, 0)} and the loss probe (with_grads = false: both losses, no backward, the probe halves of the buffers).
    //   lane 0: batch assembly; one Adam launch per TrainState that steps (critic + Polyak, value, actor: three learning rates, the
    //           actor's own counters) and the finalize, behind both side lanes
    //   lane 1: value on [obs ; next_obs] (2B rows) -> target pair -> value loss -> value backward (obs half)
    //   lane 2: critic pair forward -> critic loss (waits for value(next_obs) on lane 1) -> critic backward; then the actor: loss weights
    //           from the pair's forward pass that already ran (target_extraction: lane 1's target pair, else this lane's critic pair) and
    //           the obs half of the value pass -> the policy over 2B rows -> weighted loss -> backward -> embedding gradient
    // A step kind that does not update a net still runs the forward passes the other one reads, forward-only.  Edges between the forked
    // lanes run 1 -> 2 only (see schedule()).
    // ---------------------------------------------------------------------------------------
    void iqld_leaf_ranges(int& a_lo, int& a_hi, int& v_lo, int& v_hi) const {
        a_lo = v_lo = 1 << 30; a_hi = v_hi = 0;
        for (const Leaf& lf : leaves) {
            if (!lf.trainable) continue;
            if (lf.name.rfind("actor/", 0) == 0) { a_lo = std::min(a_lo, lf.train_id); a_hi = std::max(a_hi, lf.train_id + 1); }
            if (lf.name.rfind("value/", 0) == 0) { v_lo = std::min(v_lo, lf.train_id); v_hi = std::max(v_hi, lf.train_id + 1); }
        }
    }
    void build_iqld_program(Program& pr, bool upd_critic, bool upd_actor, bool with_grads) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        const bool probe = !with_grads;
        const bool do_c = upd_critic || probe, do_a = upd_actor || probe;
        const bool gc = upd_critic && with_grads, ga = upd_actor && with_grads;
        const bool te = dcfg.target_extraction != 0;
        DevState* st = d_state;
        float* out = iql_info + (probe ? IQLD_INFO_STRIDE : 0);
        float* rows = rows_buf + (probe ? (size_t)3 * B : 0);
        const void *I_V = &st->info[IFQL_I_VALUE], *I_C = out + IQLD_I_CRITIC, *I_W = out + IQLD_I_ACTOR, *I_A = out + IQLD_I_ACTOR + 1;
        const Net& na = nets[NET_BC];
        wide_tiles = true;
        allow64 = true;
        emit_lane = 0;
        if (do_c || do_a) {
            const IqldPrepArgs dprep{d_src, st, seed, d_emb, P + emb_off, B, od, ad, nets[NET_OS].in_p(), nets[NET_C0].in_p(), na.in_p(), ap,
                                     bc_steps, X_v, X_c1, X_bc, vel, w_rew, w_mask};
            emit(pr, OP_IQLD_PREP, bind(fql_iqld_prep_kernel, (dprep.B + 3) / 4, dprep), {P + emb_off}, {X_v, X_c1, X_bc, vel, w_rew, w_mask});
            emit_lane = 1;
            emit_forward(pr, p_v, gc);                                              // value(obs) :109,131; value(next_obs) :96
            if (do_c || te) for (int e = 0; e < 2; ++e) emit_forward(pr, p_ct[e], false);   // target_critic(obs, actions) :107,133
        }
        if (do_c) {
            const IfqlValueArgs iv{p_v.out, p_ct[0].out, p_ct[1].out, gc ? p_v.dz.back() : nullptr, st, B, dcfg.expectile};
            Op& op = emit(pr, OP_IFQL_LOSS_V, bind(fql_ifql_loss_value_kernel, 1, iv), {p_v.out, p_ct[0].out, p_ct[1].out}, {I_V});
            if (gc) op.writes.push_back(p_v.dz.back());
            if (gc) emit_backward(pr, p_v, 0, B, true, false);
        }
        emit_lane = 2;
        if (do_c || (do_a && !te)) for (int e = 0; e < 2; ++e) emit_forward(pr, p_c1[e], gc);   // critic(obs, actions) :98,135
        if (do_c) {
            const IqldCriticArgs dc{p_v.out + (size_t)B * nets[NET_OS].layers.back().out_p, p_c1[0].out, p_c1[1].out, w_rew, w_mask,
                                    gc ? p_c1[0].dz.back() : nullptr, gc ? p_c1[1].dz.back() : nullptr, out, B, cfg.discount};
            Op& op = emit(pr, OP_IQLD_LOSS_C, bind(fql_iqld_loss_critic_kernel, 1, dc), {p_v.out, p_c1[0].out, p_c1[1].out, w_rew, w_mask}, {I_C});
            if (gc) { op.writes.push_back(p_c1[0].dz.back()); op.writes.push_back(p_c1[1].dz.back()); }
            if (gc) for (int e = 0; e < 2; ++e) emit_backward(pr, p_c1[e], 0, B, true, false);
        }
        if (do_a) {
            const PassBuf* pq = te ? p_ct : p_c1;
            const IqldWeightArgs dw{pq[0].out, pq[1].out, p_v.out, w_lw, rows, out, B, dcfg.optimal_var, (int)(0.1 * (double)B),
                                    dcfg.optimal_var == IQLD_BINARY_SOFTMAX ? dcfg.softmax_beta : dcfg.awr_temperature};
            emit(pr, OP_IQLD_WEIGHT, bind(fql_iqld_weight_kernel, 1, dw), {pq[0].out, pq[1].out, p_v.out}, {w_lw, rows + (size_t)B, I_W});
            emit_forward(pr, p_bc, ga);                                             // actor(obs, 1, x_t, t) :181 and actor(obs, 0, x_t, t) :186
            {
                const IqldActorLossArgs dla{p_bc.out, vel, w_lw, ga ? p_bc.dz.back() : nullptr, rows, out, B, ad, ap};
                // (I_W: the two kernels write disjoint slots of one info block, in this order)
                Op& op = emit(pr, OP_IQLD_LOSS_A, bind(fql_iqld_loss_actor_kernel, 1, dla), {p_bc.out, vel, w_lw, I_W}, {rows, I_A});
                if (ga) op.writes.push_back(p_bc.dz.back());
            }
            if (ga) {
                emit_backward(pr, p_bc, 0, 2 * B, true, false);
                const Layer& l0 = na.layers[0];
                const IqldEmbedGradArgs deg{p_bc.dz[0], P + l0.w + (size_t)(od + ad + BC_EMB) * l0.out_p, G + emb_off, B, l0.out_p};
                emit(pr, OP_IQLD_EGRAD, bind(fql_iqld_embed_grad_kernel, 2, deg), {p_bc.dz[0], P + l0.w}, {G + emb_off});
            }
        }
        if (gc) {
            AdamOpt ao;
            ao.lr = dcfg.critic_lr;
            adam_for(pr, 2, {NET_C0, NET_C1}, 0, -1, ao);  // critic_lr; Polyak from the pre-step critic (:230)
            ao.lr = dcfg.value_lr;
            adam_for(pr, 1, {NET_OS}, 0, -1, ao);          // value_lr
        }
        if (ga) {
            AdamOpt ao;
            ao.lr = dcfg.actor_lr;
            ao.st = d_state_a;                             // the actor TrainState's own count
            Op& a = adam_for(pr, 0, {NET_BC}, 0, -1, ao);
            a.reads.push_back(G + emb_off);
            a.writes.push_back(P + emb_off);
        }
        int a_lo, a_hi, v_lo, v_hi;
        iqld_leaf_ranges(a_lo, a_hi, v_lo, v_hi);
        const IqldFinalizeArgs dfin{st, d_state_a, d_partials, d_leaf_range, out, ga ? a_lo : (gc ? v_lo : 0), ga ? a_hi : (gc ? v_hi : 0),
                                    do_c ? 1 : 0, do_a ? 1 : 0, gc ? 1 : 0, ga ? 1 : 0, with_grads ? 1 : 0};
        emit_fin(pr, OP_IQLD_FIN, bind(fql_iqld_finalize_kernel, 1, dfin), -1, {I_V, I_C, I_W, I_A}, with_grads, {out, st, d_state_a});
    }

    void build_iqld_workspace() {
        const int ap = pad16(cfg.act_dim);
        auto& W = ws_allocs;
        X_v = dalloc(W, (size_t)2 * B * nets[NET_OS].in_p());
        X_c1 = dalloc(W, (size_t)B * nets[NET_C0].in_p());
        X_bc = dalloc(W, (size_t)2 * B * nets[NET_BC].in_p());
        vel = dalloc(W, (size_t)B * ap);
        w_rew = dalloc(W, B); w_mask = dalloc(W, B); w_lw = dalloc(W, B);
        rows_buf = dalloc(W, (size_t)6 * B);
        p_v = make_pass(W, NET_OS, 2 * B, X_v, true, false);
        p_bc = make_pass(W, NET_BC, 2 * B, X_bc, true, false);
        for (int e = 0; e < 2; ++e) {
            p_c1[e] = make_pass(W, NET_C0 + e, B, X_c1, true, false);
            p_ct[e] = make_pass(W, NET_T0 + e, B, X_c1, false, false);
        }
        build_iqld_program(prog_full, true, true, true);
        build_iqld_program(prog_critic, true, false, true);
        build_iqld_program(prog_actor, false, true, true);
        build_iqld_program(prog_none, false, false, true);
        build_iqld_program(prog_loss, false, false, false);
        finish_programs({&prog_full, &prog_critic, &prog_actor, &prog_none, &prog_loss});
    }
    Program& iqld_program(bool upd_critic, bool upd_actor) {
        return upd_critic ? (upd_actor ? prog_full : prog_critic) : (upd_actor ? prog_actor : prog_none);
    }
    // multiply-accumulates of one IQL-diffusion update per batch row, algorithmic (full GEMM shapes at the logical widths)
    int64_t iqld_macs(bool upd_critic, bool upd_actor) const {
        const int64_t va = net_macs(nets[NET_OS]), ac = net_macs(nets[NET_BC]), cr = net_macs(nets[NET_C0]);
        const bool te = dcfg.target_extraction != 0;
        int64_t m = 0;
        if (upd_critic || upd_actor) m += 2 * va;                                  // value on 2B rows
        if (upd_critic || (upd_actor && te)) m += 2 * cr;                          // target pair
        if (upd_critic || (upd_actor && !te)) m += 2 * cr;                         // critic pair
        if (upd_critic) m += (2 * va - first_macs(nets[NET_OS])) + 2 * (2 * cr - first_macs(nets[NET_C0]));
        if (upd_actor) m += 2 * ac + 2 * (2 * ac - first_macs(nets[NET_BC]));      // the policy on 2B rows, forward + backward
        return m * (int64_t)B;
    }

    // multiply-accumulates of one ReBRAC update per batch row, algorithmic (full GEMM shapes)
    int64_t rebrac_macs(bool full_update) const {
        const int64_t ac = net_macs(nets[NET_BC]), cr = net_macs(nets[NET_C0]);
        // target actor + target pair forward; critic pair forward + backward without the input gradient
        int64_t m = ac + 2 * cr + 2 * cr + 2 * (2 * cr - first_macs(nets[NET_C0]));
        // actor forward; the pair on [obs | a] forward + input gradient; actor backward without the input gradient
        if (full_update) m += ac + 2 * cr + 2 * cr + (2 * ac - first_macs(nets[NET_BC]));
        return m * (int64_t)B;
    }

    int64_t macs_per_update() const { return desc().macs(*this); }   // (of the kind's full update)
    // multiply-accumulates of one IFQL update: value on 2B rows + its backward on B; target pair; critic pair forward + backward (no input
    // gradient); actor_flow forward + backward
    int64_t ifql_macs() const {
        const int64_t os = net_macs(nets[NET_OS]), bc = net_macs(nets[NET_BC]), cr = net_macs(nets[NET_C0]);
        const int64_t fwd = 2 * os + 4 * cr + bc;
        const int64_t bwd = (2 * os - first_macs(nets[NET_OS])) + 2 * (2 * cr - first_macs(nets[NET_C0])) + (2 * bc - first_macs(nets[NET_BC]));
        return (fwd + bwd) * (int64_t)B;
    }
    int64_t fql_macs() const {
        const int64_t os = net_macs(nets[NET_OS]), bc = net_macs(nets[NET_BC]), cr = net_macs(nets[NET_C0]);
        const int64_t fwd = 3 * os + (cfg.flow_steps + 1) * bc + 6 * cr;
        const int64_t bwd = 2 * (2 * cr - first_macs(nets[NET_C0])) + (2 * bc - first_macs(nets[NET_BC])) + (2 * os - first_macs(nets[NET_OS])) + 2 * cr;
        int64_t total = (fwd + bwd) * (int64_t)B;
        if (visual) {
            // encoder: 5 distinct forward image-batches per update (onestep on obs and next_obs, critic, target, bc_flow; the
            // reference's other three encoder calls repeat one of these on the same images and parameters) and 3 backward
            // passes = dgrad (none into the images) + wgrad; plus the MLPs' layer-0 input gradients that feed them
            const EncNet& en = encs[ENC_C];
            int64_t f = (int64_t)en.dense.in * en.dense.out, first_conv = 0;
            for (size_t s = 0; s < en.stacks.size(); ++s)
                for (size_t j = 0; j < en.stacks[s].conv.size(); ++j) {
                    const ConvL& c = en.stacks[s].conv[j];
                    const int H = j == 0 ? en.stacks[s].H : en.stacks[s].H / 2, W = j == 0 ? en.stacks[s].W : en.stacks[s].W / 2;
                    const int64_t m = (int64_t)H * W * 9 * c.cin * c.cout;
                    f += m;
                    if (s == 0 && j == 0) first_conv = m;
                }
            total += (int64_t)B * (5 * f + 3 * (2 * f - first_conv));
            total += (int64_t)B * enc_dim * (2 * (int64_t)nets[NET_C0].layers[0].out + nets[NET_BC].layers[0].out + nets[NET_OS].layers[0].out);
        }
        return total;
    }

    void free_workspace() noexcept {
        free_program(prog_fwdbwd);
        free_program(prog_opt);
        free_program(prog_opt_split);
        free_program(prog_loss);
        free_program(prog_split);
        free_program(prog_full);
        free_program(prog_critic);
        free_program(prog_actor);
        free_program(prog_none);
        free_split();
        for (void* p : ws_allocs) hipFree(p);
        ws_allocs.clear();
    }

    void build_workspace(int batch) {
        if (batch <= 0 || batch % 16 != 0) invalid("batch_size must be a positive multiple of 16 (got %d)", batch);
        HIP_CHECK(hipStreamSynchronize(stream));
        free_workspace();
        B = batch;
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        auto& W = ws_allocs;
        in_obs = dalloc(W, (size_t)B * od); in_nobs = dalloc(W, (size_t)B * od);
        in_act = dalloc(W, (size_t)B * ad); in_rew = dalloc(W, B); in_mask = dalloc(W, B);
        for (int i = 0; i < 5; ++i) in_noise[i] = dalloc(W, (size_t)B * ad);
        in_idx = (int64_t*)dalloc(W, (size_t)B * 4);   // [2][B]: indices in use, staging of host indices (frames path)
        (this->*desc().workspace)();
    }
    void build_fql_workspace() {
        const int ad = cfg.act_dim;
        auto& W = ws_allocs;
        const int inp_c = nets[NET_OS].in_p(), inp_b = nets[NET_BC].in_p();
        X_os = dalloc(W, (size_t)3 * B * inp_c); X_bc = dalloc(W, (size_t)B * inp_b); X_eu = dalloc(W, (size_t)B * inp_b);
        X_c1 = dalloc(W, (size_t)B * inp_c); X_c2 = dalloc(W, (size_t)B * inp_c); X_ct = dalloc(W, (size_t)B * inp_c);
        const int ap = pad16(ad);
        vel = dalloc(W, (size_t)B * ap); w_act = dalloc(W, (size_t)B * ap); tgt = dalloc(W, (size_t)B * ap);
        w_rew = dalloc(W, B); w_mask = dalloc(W, B);
        {   // fused Euler chain (layers 0+1 and last-hidden+head per launch): plain actor MLPs with >= 2 hidden layers
            const Net& nb = nets[NET_BC];
            const int nh = nb.nl() - 1;
            fused_euler = !cfg.actor_layer_norm && ad <= 15 && nh >= 3;   // 16-wide rank update: act + t
            if (fused_euler) {
                X_e0 = dalloc(W, (size_t)B * inp_b);
                C0 = dalloc(W, (size_t)B * nb.layers[0].out_p);
                Abuf[0] = dalloc(W, (size_t)B * ap); Abuf[1] = dalloc(W, (size_t)B * ap);
                vp_tiles = (nb.layers[nh - 1].out_p / 16 + 1) / 2;
                if (vp_tiles > 32) fused_euler = false;
                Vpart = dalloc(W, (size_t)std::max(vp_tiles, 1) * B * ap);
            }
        }
        if (visual) {
            const size_t ib = (size_t)cfg.img_h * cfg.img_w * cfg.img_c;
            img_all = (unsigned char*)dalloc(W, (2 * (size_t)B * ib + 3) / 4 + 4);
            in_init = (int64_t*)dalloc(W, (size_t)B * 2);
            in_crop = (int*)dalloc(W, (size_t)B * 2); in_crop_user = (int*)dalloc(W, (size_t)B * 2);
            eb_os = make_enc_buf(W, ENC_OS, 2 * B, img_all, true);
            eb_c = make_enc_buf(W, ENC_C, B, img_all, true);
            eb_t = make_enc_buf(W, ENC_T, B, img_all + (size_t)B * ib, false);
            eb_bc = make_enc_buf(W, ENC_BC, B, img_all, true);
        }
        p_os = make_pass(W, NET_OS, 3 * B, X_os, false, false);
        {   // backward view of the (obs, z) block: own gradient buffers, forward buffers shared with p_os
            p_os_bwd = p_os;
            p_os_bwd.M = B;
            const Net& n = nets[NET_OS];
            for (int l = 0; l < n.nl(); ++l) p_os_bwd.dz.push_back(dalloc(W, (size_t)B * n.layers[l].out_p));
            for (int l = 0; l + 1 < n.nl(); ++l) p_os_bwd.dy.push_back(n.layers[l].ln ? dalloc(W, (size_t)B * n.layers[l].out_p) : nullptr);
            if (visual) p_os_bwd.dx0 = dalloc(W, (size_t)B * n.in_p());
        }
        p_bc = make_pass(W, NET_BC, B, X_bc, true, visual);
        p_eu = make_pass(W, NET_BC, B, X_eu, false, false);
        for (int e = 0; e < 2; ++e) {
            p_c1[e] = make_pass(W, NET_C0 + e, B, X_c1, true, visual);
            p_c2[e] = make_pass(W, NET_C0 + e, B, X_c2, true, true);
            p_ct[e] = make_pass(W, NET_T0 + e, B, X_ct, false, false);
        }
        if (!cfg.normalize_q_loss) {
            std::vector<float> h((size_t)B * 16, 0.f);
            for (int b = 0; b < B; ++b) h[(size_t)b * 16] = -1.0f / (2.0f * (float)B);
            for (int e = 0; e < 2; ++e) HIP_CHECK(hipMemcpy(p_c2[e].dz.back(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        static const bool trace = getenv("FQL_TRACE") != nullptr;
#define FQL_TR(msg) do { if (trace) fprintf(stderr, "[fql] %s\n", msg); } while (0)
        build_step_program(prog_fwdbwd, true);
        build_opt_program(prog_opt, false);
        build_opt_program(prog_opt_split, true);
        build_step_program(prog_loss, false);
        FQL_TR("programs built");
        schedule(prog_fwdbwd, W); FQL_TR("scheduled fwdbwd"); schedule(prog_opt, W); schedule(prog_opt_split, W); schedule(prog_loss, W);
        FQL_TR("scheduled");
        capture(prog_fwdbwd); FQL_TR("captured fwdbwd"); capture(prog_opt); capture(prog_loss);
        FQL_TR("captured");
        {
            build_full_program(prog_full);
            schedule(prog_full, W);
            FQL_TR("scheduled full");
            capture(prog_full);
            FQL_TR("captured full");
        }
        {
            split_build = true;
            build_step_program(prog_split, true);
            split_build = false;
            schedule(prog_split, W);
            split_ok = capture_split(prog_split);
        }
        src_valid = false;
    }

    // ---------------------------------------------------------------------------------------
    // inputs
    // ---------------------------------------------------------------------------------------
    static bool is_device_ptr(const void* p) {
        hipPointerAttribute_t a;
        hipError_t e = hipPointerGetAttributes(&a, p);
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeUnified;
    }
    bool staged_host = false;
    // host memory is borrowed for the call only: drain the staging copies before returning
    void drain_staging(hipStream_t s) {
        if (staged_host) { HIP_CHECK(hipStreamSynchronize(s)); staged_host = false; }
    }
    // HIP is about to write a buffer the update reads: updates still on the AQL queues must have finished, and the next AQL submit must wait for the stream
    void hip_touch() { aql_drain(); hip_dirty = true; }
    const float* stage(const float* p, float* staging, size_t n, hipStream_t s) {
        if (!p) return nullptr;
        if (is_device_ptr(p)) return p;
        hip_touch();
        HIP_CHECK(hipMemcpyAsync(staging, p, n * sizeof(float), hipMemcpyHostToDevice, s));
        staged_host = true;
        return staging;
    }
    void set_source(const SrcDesc& d, hipStream_t s) {
        if (src_valid && std::memcmp(&d, &h_src_shadow, sizeof d) == 0) return;
        SrcDesc* slot = &h_src_ring[src_ring_pos];
        src_ring_pos = (src_ring_pos + 1) % 64;
        *slot = d;
        hip_touch();
        HIP_CHECK(hipMemcpyAsync(d_src, slot, sizeof d, hipMemcpyHostToDevice, s));
        h_src_shadow = d;
        src_valid = true;
    }
    void source_from_batch(const float* obs, const float* act, const float* rew, const float* mask, const float* nobs,
                           int batch, const fql_noise* nz, int advance, hipStream_t s) {
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d); call fql_set_batch_size", batch, B);
        if (!obs || !act || !rew || !mask || !nobs) invalid("batch pointers must not be NULL");
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        SrcDesc d{};
        if (visual) {   // uint8 [B, H, W, C] batches into the fixed image buffer the encoder launches read: [obs ; next_obs]
            const size_t ib = (size_t)cfg.img_h * cfg.img_w * cfg.img_c;
            HIP_CHECK(hipMemcpyAsync(img_all, obs, (size_t)B * ib, hipMemcpyDefault, s));
            HIP_CHECK(hipMemcpyAsync(img_all + (size_t)B * ib, nobs, (size_t)B * ib, hipMemcpyDefault, s));
            if (!is_device_ptr(obs) || !is_device_ptr(nobs)) staged_host = true;
        } else {
            d.obs = stage(obs, in_obs, (size_t)B * od, s);
            d.nobs = stage(nobs, in_nobs, (size_t)B * od, s);
        }
        d.act = stage(act, in_act, (size_t)B * ad, s);
        d.rew = stage(rew, in_rew, B, s);
        d.mask = stage(mask, in_mask, B, s);
        fill_noise(d, nz, s);
        d.advance = advance;
        drain_staging(s);
        set_source(d, s);
    }
    // BC batches carry observations and actions only (agents/bc.py:56-69)
    void bc_source_from_batch(const float* obs, const float* act, int batch, const fql_noise* nz, int advance, hipStream_t s) {
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d); call fql_set_batch_size", batch, B);
        if (!obs || !act) invalid("batch pointers must not be NULL");
        SrcDesc d{};
        d.obs = stage(obs, in_obs, (size_t)B * cfg.obs_dim, s);
        d.act = stage(act, in_act, (size_t)B * cfg.act_dim, s);
        fill_noise(d, nz, s);
        d.advance = advance;
        drain_staging(s);
        set_source(d, s);
    }
    void drop_goal_table() {   // the dataset's rows changed: the per-row `final` table and the representations no longer describe them
        if (!ds_final && !ds_reps) return;
        hipFree(ds_final); hipFree(ds_reps);
        ds_final = nullptr; ds_reps = nullptr;
        gsrc_valid = false;
    }
    // CFGRL: where the goals and the mask of the next step come from (CfgrlSrc), rewritten when it changes as set_source does
    void set_goal_source(const CfgrlSrc& g, hipStream_t s) {
        if (gsrc_valid && std::memcmp(&g, &h_gsrc_shadow, sizeof g) == 0) return;
        CfgrlSrc* slot = &h_gsrc_ring[gsrc_ring_pos];
        gsrc_ring_pos = (gsrc_ring_pos + 1) % 64;
        std::memcpy(slot, &g, sizeof g);
        hip_touch();
        HIP_CHECK(hipMemcpyAsync(d_gsrc, slot, sizeof g, hipMemcpyHostToDevice, s));
        std::memcpy(&h_gsrc_shadow, &g, sizeof g);
        gsrc_valid = true;
    }
    CfgrlSrc goal_source(const float* goals, const unsigned char* do_cfg, hipStream_t s) {
        CfgrlSrc g;
        std::memset(&g, 0, sizeof g);   // (padding bytes too: set_goal_source compares the bytes)
        g.goals = stage(goals, in_goal, (size_t)B * gcfg.goal_dim, s);
        if (do_cfg) {
            if (is_device_ptr(do_cfg)) g.do_cfg = do_cfg;
            else {
                hip_touch();
                HIP_CHECK(hipMemcpyAsync(in_cfg, do_cfg, (size_t)B, hipMemcpyHostToDevice, s));
                staged_host = true;
                g.do_cfg = in_cfg;
            }
        }
        g.final_idx = ds_final;
        g.reps = ds_reps ? ds_reps : ds_obs;
        g.n = ds_size;
        g.all_cur = gcfg.actor_p_curgoal == 1.0 ? 1 : 0;
        g.thr_traj = g.all_cur ? 0.0 : gcfg.actor_p_trajgoal / (1.0 - gcfg.actor_p_curgoal);   // utils/datasets.py:249
        g.p_cur = gcfg.actor_p_curgoal;
        g.thr_mask = (uint64_t)(gcfg.p_uncond * 4294967296.0);
        return g;
    }
    // CFGRL batches carry observations, actions and actor_goals (agents/cfgrl.py:24-37); do_cfg: [B] bytes or null (engine RNG)
    void cfgrl_source_from_batch(const float* obs, const float* act, const float* goals, const unsigned char* do_cfg, int batch,
                                 const fql_noise* nz, int advance, hipStream_t s) {
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d); call fql_set_batch_size", batch, B);
        if (!obs || !act || !goals) invalid("batch pointers must not be NULL (CFGRL batches carry actor_goals)");
        SrcDesc d{};
        d.obs = stage(obs, in_obs, (size_t)B * cfg.obs_dim, s);
        d.act = stage(act, in_act, (size_t)B * cfg.act_dim, s);
        fill_noise(d, nz, s);
        d.advance = advance;
        const CfgrlSrc g = goal_source(goals, do_cfg, s);
        drain_staging(s);
        set_source(d, s);
        set_goal_source(g, s);
    }
    // GCDataset.sample on the device: the index draw of every update_from_dataset, then the goal of each row from its own trajectory
    void cfgrl_source_from_dataset(const int64_t* idx, int batch, int64_t lo, int64_t hi, const fql_noise* nz, const unsigned char* do_cfg,
                                   hipStream_t s) {
        if (!ds_final) throw Invalid{"fql_cfgrl_update_from_dataset: no goal table (fql_cfgrl_dataset_goals after fql_dataset_upload)"};
        source_from_dataset(idx, batch, lo, hi, nz, s);
        const CfgrlSrc g = goal_source(nullptr, do_cfg, s);
        drain_staging(s);
        set_goal_source(g, s);
    }
    void fill_noise(SrcDesc& d, const fql_noise* nz, hipStream_t s) {
        const int ad = cfg.act_dim;
        if (!nz) return;
        const int given = (nz->eps1 ? NZ_EPS1 : 0) | (nz->x0 ? NZ_X0 : 0) | (nz->t ? NZ_T : 0) | (nz->z ? NZ_Z : 0) | (nz->eps2 ? NZ_EPS2 : 0);
        if (given & ~desc().noise_reads) invalid("%s", desc().noise_refusal);
        if (has(K_TIME_TABLE) && nz->t && !is_device_ptr(nz->t))   // t = k / S on the grid (device pointers are the caller's to keep on it: read as round(t S))
            for (int b = 0; b < B; ++b) {
                const float ts = nz->t[b] * (float)bc_steps;
                if (!(ts >= -1e-3f && ts <= (float)bc_steps + 1e-3f) || std::fabs(ts - std::nearbyint(ts)) > 1e-3f)
                    invalid("%s: t[%d] = %g is not on the grid {0, 1/%d, ..., 1}", desc().name, b, (double)nz->t[b], bc_steps);
            }
        d.eps1 = stage(nz->eps1, in_noise[0], (size_t)B * ad, s);
        d.x0 = stage(nz->x0, in_noise[1], (size_t)B * ad, s);
        d.t = stage(nz->t, in_noise[2], B, s);
        d.z = stage(nz->z, in_noise[3], (size_t)B * ad, s);
        d.eps2 = stage(nz->eps2, in_noise[4], (size_t)B * ad, s);
    }
    void source_from_dataset(const int64_t* idx, int batch, int64_t lo, int64_t hi, const fql_noise* nz, hipStream_t s) {
        if (visual) { source_from_frames(idx, nullptr, batch, lo, hi, nz, s); return; }
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d)", batch, B);
        if (!ds_obs || ds_size <= 0) throw Invalid{"no dataset uploaded (fql_dataset_upload)"};
        if (lo == 0 && hi == 0) hi = ds_size;
        if (lo < 0 || hi > ds_size || lo >= hi) invalid("bad sampling range [%lld, %lld) for dataset of %lld rows", (long long)lo, (long long)hi, (long long)ds_size);
        SrcDesc d{};
        d.obs = ds_obs; d.act = ds_act; d.rew = ds_rew; d.mask = ds_mask; d.nobs = ds_nobs;
        if (has(K_NEXT_ACTIONS)) { d.nact = ds_act; d.nact_rows = ds_size; }   // utils/datasets.py:96-100: actions[min(idx + 1, size - 1)], the whole dataset's size
        if (idx) {
            if (is_device_ptr(idx)) d.idx = idx;
            else {
                hip_touch();
                HIP_CHECK(hipMemcpyAsync(in_idx, idx, (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
                staged_host = true;
                d.idx = in_idx;
            }
        } else {
            d.use_rng_idx = 1; d.lo = lo; d.span = hi - lo;
        }
        fill_noise(d, nz, s);
        d.advance = 1;
        drain_staging(s);
        set_source(d, s);
    }
    // indices of a balanced batch into one device array: rows [0, split) index the dataset, rows [split, B) the replay ring
    const int64_t* stage_two_idx(const int64_t* a, const int64_t* b, int split, int64_t* dst, hipStream_t s) {
        if (!a && !b) return nullptr;
        if (!a || !b) throw Invalid{"balanced sampling: give both index arrays or neither"};
        hip_touch();
        HIP_CHECK(hipMemcpyAsync(dst, a, (size_t)split * sizeof(int64_t), hipMemcpyDefault, s));
        HIP_CHECK(hipMemcpyAsync(dst + split, b, (size_t)(B - split) * sizeof(int64_t), hipMemcpyDefault, s));
        if (!is_device_ptr(a) || !is_device_ptr(b)) staged_host = true;
        return dst;
    }
    // main.py:255-259: batch = concat(train_dataset.sample(B // 2), replay_buffer.sample(B // 2)), gathered on the device
    void source_balanced(const int64_t* idx_ds, const int64_t* idx_rb, const int32_t* crop, int batch, const fql_noise* nz, hipStream_t s) {
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d)", batch, B);
        if (B % 2) invalid("balanced sampling draws batch_size // 2 rows from each source: batch_size %d must be even", B);
        if (ds_size <= 0 || !(visual ? (void*)ds_frames : (void*)ds_obs)) throw Invalid{"balanced sampling: no training dataset uploaded"};
        if (rb_cap <= 0) throw Invalid{"balanced sampling: no replay ring (fql_replay_create)"};
        if (rb_size <= 0) throw Invalid{"balanced sampling: the replay ring is empty (the reference would draw randint(0), a ValueError)"};
        const int split = B / 2;
        if (visual) { source_from_frames(idx_ds, crop, batch, 0, 0, nz, s, split, idx_rb); return; }
        SrcDesc d{};
        d.obs = ds_obs; d.act = ds_act; d.rew = ds_rew; d.mask = ds_mask; d.nobs = ds_nobs;
        d.obs2 = rb_obs; d.act2 = rb_act; d.rew2 = rb_rew; d.mask2 = rb_mask; d.nobs2 = rb_nobs;
        d.split = split;
        d.idx = stage_two_idx(idx_ds, idx_rb, split, in_idx, s);
        if (!d.idx) { d.use_rng_idx = 1; d.lo = 0; d.span = ds_size; d.lo2 = 0; d.span2 = rb_size; }
        fill_noise(d, nz, s);
        d.advance = 1;
        drain_staging(s);
        set_source(d, s);
    }
    // Dataset.sample for image datasets (utils/datasets.py:68-92): indices, frame stacking, random crop -> img_all, on the device
    void source_from_frames(const int64_t* idx, const int32_t* crop, int batch, int64_t lo, int64_t hi, const fql_noise* nz, hipStream_t s,
                            int split = 0, const int64_t* idx_rb = nullptr) {
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d)", batch, B);
        if (!visual || !ds_frames || ds_size <= 0) throw Invalid{"no frames dataset uploaded (fql_dataset_upload_frames)"};
        if (lo == 0 && hi == 0) hi = ds_size;
        if (lo < 0 || hi > ds_size || lo >= hi) invalid("bad sampling range [%lld, %lld) for dataset of %lld rows", (long long)lo, (long long)hi, (long long)ds_size);
        const int64_t* idx_dev = nullptr;
        if (split > 0) {
            if (!rb_frames) throw Invalid{"balanced sampling: the replay ring holds no frames"};
            idx_dev = stage_two_idx(idx, idx_rb, split, in_idx + B, s);
        } else if (idx) {
            if (is_device_ptr(idx)) idx_dev = idx;
            else {
                HIP_CHECK(hipMemcpyAsync(in_idx + B, idx, (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));   // second half of in_idx
                staged_host = true;
                idx_dev = in_idx + B;
            }
        }
        const int* crop_dev = nullptr;
        if (crop) {
            if (is_device_ptr(crop)) crop_dev = crop;
            else {
                HIP_CHECK(hipMemcpyAsync(in_crop_user, crop, (size_t)B * 2 * sizeof(int), hipMemcpyHostToDevice, s));
                staged_host = true;
                crop_dev = in_crop_user;
            }
        }
        ImgIndexArgs ia{idx_dev, crop_dev, ds_init, d_state, seed, lo, hi - lo, ds_paug, B, 3, in_idx, in_init, in_crop,
                        split, rb_init, 0, rb_size};
        hipLaunchKernelGGL(fql_img_index_kernel, dim3((B + FQL_THREADS - 1) / FQL_THREADS), dim3(FQL_THREADS), 0, s, ia);
        const size_t ib = (size_t)cfg.img_h * cfg.img_w * cfg.img_c;
        ImgGatherArgs ga{ds_frames, ds_next_frames, in_idx, in_init, in_crop, img_all, img_all + (size_t)B * ib,
                         B, cfg.img_h, cfg.img_w, cfg.img_c / ds_fs, ds_fs, 3, split, rb_frames, rb_next_frames};
        const size_t tot = ((size_t)B * ib) >> 2;   // one thread per four output bytes (img_w is a multiple of 32: rows are whole dwords)
        hipLaunchKernelGGL(fql_img_gather_kernel, dim3((unsigned)((tot + FQL_THREADS - 1) / FQL_THREADS)), dim3(FQL_THREADS), 0, s, ga);
        HIP_CHECK(hipGetLastError());
        SrcDesc d{};
        d.act = ds_act; d.rew = ds_rew; d.mask = ds_mask;
        d.idx = in_idx;
        if (split > 0) { d.split = split; d.act2 = rb_act; d.rew2 = rb_rew; d.mask2 = rb_mask; }
        fill_noise(d, nz, s);
        d.advance = 1;
        drain_staging(s);
        set_source(d, s);
    }
    // where the infos of the last update are: DevState::info, or an IQL handle's own buffer
    const float* info_src() const { return own_info() ? iql_info : &d_state->info[0]; }
    void finish_info(float* info, int n, hipStream_t s) {
        if (!info) return;
        hip_touch();
        if (is_device_ptr(info)) {
            HIP_CHECK(hipMemcpyAsync(info, info_src(), n * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            HIP_CHECK(hipMemcpyAsync(info, info_src(), n * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
    }

    // ---------------------------------------------------------------------------------------
    // eval paths
    // ---------------------------------------------------------------------------------------
    // the kind's FlowShape on this handle: the row's halves, shared_x and tables; the steps and the goal block; a sweep where there is a guidance weight
    FlowShape flow_shape(bool sweep) const {
        FlowShape sh = desc().flow;
        sh.S = has(K_GOALS) ? gcfg.flow_steps : bc_steps;
        sh.goal_dim = has(K_GOALS) ? gcfg.goal_dim : 0;
        sh.sweep = sweep && sh.halves == 2;
        return sh;
    }
    // the loop-invariant layer-0 term of a hoisted flow sampler: C0 = X W0 + b0 over `rows` rows
    void emit_c0(Program& pr, const float* X, int rows, float* C0e) {
        const Layer& l0 = nets[NET_BC].layers[0];
        Op op{};
        op.type = OP_GEMM;
        GemmTask& t = op.gemm;
        t.A = X; t.lda = l0.in_p; t.B = P + l0.w; t.ldb = l0.out_p; t.bias = P + l0.b; t.C = C0e; t.ldc = l0.out_p;
        t.M = rows; t.N = l0.out_p; t.K = l0.in_p; t.flags = GF_BIAS;
        op.reads = {X, t.B};
        op.writes = {C0e};
        push(pr, op);
    }
    // sample_actions of the flow policies (prog_flow), hoisted: the step-bias table (BC, IQL-diffusion) and the loop-invariant C0 at the
    // head of the program, then per Euler step layer 0 as a rank-act update of C0 plus the step's row (one launch, both halves), layers
    // 1.. of the 16-row Dense kernel over n_pad rows, and the guidance step:
    //   BC: none, the head GEMM's epilogue adds v / S to the actions in place and on the last step writes the clipped actions
    //   scalar cfg: fql_iqld_cfg_step_kernel behind every head GEMM (CFG combine + Euler add; issue() writes the call's cfg into the
    //     launch; the last one writes the clipped actions)
    //   sweep: S - 1 launches fewer.  Step 0 runs the plain layer-0 kernel on X[0], where the assemble kernel
    //     wrote x.  Step i >= 1 is ONE launch in front of its GEMMs: the combine and Euler add of step i - 1 with the row's weight, then
    //     layer 0 on the new x, which it also writes to X[i & 1] while every thread reads X[(i - 1) & 1].  Behind the last head GEMM the
    //     rows step kernel reads X[(S - 1) & 1] and writes the clipped actions.  The weights [half] are bound here; the call copies them
    //     in (sample_flow), so issue() patches nothing.
    // n_pad counts both halves of a CFG kind, half = n_pad / 2 a multiple of 16.
    void build_flow_sampler(Eval& ev, const FlowShape& sh) {
        auto& W = ev.allocs;
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad), S = sh.S, Gd = sh.goal_dim;
        const int n_pad = ev.n_pad, half = n_pad / sh.halves, rows0 = sh.shared_x ? half : n_pad;
        const Net& n = nets[NET_BC];
        const Layer& l0 = n.layers[0];
        const int H = l0.out_p;
        const float dt = 1.0f / (float)S;
        ev.X = dalloc(W, (size_t)rows0 * n.in_p());                      // [obs | 0]; CFGRL: [obs | goal | 0] ; [obs | unc_embed | 0]
        ev.Xf = dalloc(W, (size_t)half * ap);                            // the flow's state x (sweep: X[0])
        if (sh.sweep) ev.Xf2 = dalloc(W, (size_t)half * ap);             // X[1]
        if (sh.tables) ev.Xq = dalloc(W, (size_t)S * sh.tables * H);     // step-bias table c[i] / c[i][half]
        float* C0e = dalloc(W, (size_t)rows0 * H);
        ev.tgt = dalloc(W, (size_t)half * ap);
        if (sh.sweep) ev.cfgs = dalloc(W, (size_t)half);
        ev.st_obs = dalloc(W, (size_t)half * od);
        if (Gd) ev.st_goal = dalloc(W, (size_t)half * Gd);
        ev.st_noise = dalloc(W, (size_t)half * ad);
        ev.st_out = dalloc(W, (size_t)half * ad);
        ev.p_eu = make_pass(W, NET_BC, n_pad, ev.X, false, false);
        float* const Xpp[2] = {ev.Xf, ev.Xf2};
        float* const g0 = ev.p_eu.g[0];
        const float* W0a = P + l0.w + (size_t)(od + Gd) * H;   // the action rows of W0 (CFGRL: the t row behind them)
        const float* W0e = P + l0.w + (size_t)(od + ad) * H;   // BC, IQL-diffusion: the time-embedding rows behind them
        const int grid0 = (sh.halves * half * H + FQL_THREADS - 1) / FQL_THREADS;
        emit_lane = 0;
        Program& pr = ev.prog_flow;
        if (sh.tables == 1) {
            const BcStepBiasArgs bsb{d_emb, W0e, ev.Xq, S, H};
            emit(pr, OP_BC_STEPBIAS, bind(fql_bc_stepbias_kernel, (bsb.S * bsb.H + FQL_THREADS - 1) / FQL_THREADS, bsb), {d_emb, P + l0.w}, {ev.Xq});
        } else if (sh.tables == 2) {
            const IqldStepBiasArgs dsb{d_emb, P + emb_off, W0e, ev.Xq, S, H};
            emit(pr, OP_IQLD_STEPBIAS, bind(fql_iqld_stepbias_kernel, (dsb.S * 2 * dsb.H + FQL_THREADS - 1) / FQL_THREADS, dsb),
                 {d_emb, P + emb_off, P + l0.w}, {ev.Xq});
        }
        emit_c0(pr, ev.X, rows0, C0e);
        for (int i = 0; i < S; ++i) {
            const bool last = i == S - 1;
            const float ti = (float)((double)i / (double)S);   // cfgrl.py:90: a Python float, cast to fp32
            const float* cb = sh.tables ? ev.Xq + (size_t)i * sh.tables * H : nullptr;
            Op* op;
            if (!sh.sweep || i == 0) {   // layer 0 on x = Xf
                const OpType ty = sh.tables == 1 ? OP_BC_LAYER0 : sh.tables == 2 ? OP_IQLD_LAYER0 : OP_CFGRL_LAYER0;
                const Bound k = sh.tables == 1   ? bind(fql_bc_layer0_kernel, grid0, BcLayer0Args{C0e, ev.Xf, W0a, cb, g0, half, H, ad, ap})
                                : sh.tables == 2 ? bind(fql_iqld_layer0_kernel, grid0, IqldLayer0Args{C0e, ev.Xf, W0a, cb, g0, half, H, ad, ap})
                                                 : bind(fql_cfgrl_layer0_kernel, grid0, CfgrlLayer0Args{C0e, ev.Xf, W0a, g0, half, H, ad, ap, ti});
                op = &emit(pr, ty, k, {C0e, ev.Xf, P + l0.w}, {g0});
            } else {
                float *xin = Xpp[(i - 1) & 1], *xout = Xpp[i & 1];
                const Bound k = sh.tables ? bind(fql_iqld_cfg_layer0_kernel, grid0,
                                                 IqldCfgLayer0Args{C0e, ev.p_eu.out, xin, ev.cfgs, W0a, cb, xout, g0, half, H, ad, ap, dt})
                                          : bind(fql_cfgrl_cfg_layer0_kernel, grid0,
                                                 CfgrlCfgLayer0Args{C0e, ev.p_eu.out, xin, ev.cfgs, W0a, xout, g0, half, H, ad, ap, ti, dt});
                op = &emit(pr, OP_CFG_ROWS_LAYER0, k, {C0e, ev.p_eu.out, xin, ev.cfgs, P + l0.w}, {g0, xout});
            }
            if (sh.tables) op->reads.push_back(ev.Xq);
            if (sh.halves == 1) {
                emit_forward(pr, ev.p_eu, false, GF_EULER | (last ? GF_EULER_LAST : 0), ev.Xf, ev.tgt, dt, 0.f, 1);
                GemmTask& hd = pr.ops.back().gemm;   // the actions alone: ld ap, no observation block in front, no time block behind
                hd.flags |= GF_EULER_BARE;
                hd.i0 = ap; hd.i1 = 0;
                continue;
            }
            emit_forward(pr, ev.p_eu, false, 0, nullptr, nullptr, 0.f, 0.f, 1);
            if (!sh.sweep) {
                const IqldCfgStepArgs dstep{ev.p_eu.out, ev.Xf, last ? ev.tgt : nullptr, half, ad, ap, 1.0f, dt};
                Op& st = emit(pr, OP_IQLD_CFG, bind(fql_iqld_cfg_step_kernel, (dstep.n_pad * dstep.ad + FQL_THREADS - 1) / FQL_THREADS, dstep),
                              {ev.p_eu.out}, {ev.Xf});
                if (last) st.writes.push_back(ev.tgt);
            } else if (last) {
                const IqldCfgRowsStepArgs dstep{ev.p_eu.out, Xpp[i & 1], ev.cfgs, ev.tgt, half, ad, ap, dt};
                emit(pr, OP_CFG_ROWS_STEP, bind(fql_iqld_cfg_rows_step_kernel, (dstep.n_pad * dstep.ad + FQL_THREADS - 1) / FQL_THREADS, dstep),
                     {ev.p_eu.out, dstep.X, ev.cfgs}, {ev.tgt});
            }
        }
        schedule(pr, W);
    }
    // ReBRAC, SAC, IQL sample_actions: the actor's forward over the rows (prog_os on p_os; NET_OS is empty here)
    void build_actor_eval(Eval& ev) {
        auto& W = ev.allocs;
        const int od = cfg.obs_dim, ad = cfg.act_dim, n_pad = ev.n_pad;
        ev.X = dalloc(W, (size_t)n_pad * nets[NET_BC].in_p());
        ev.st_obs = dalloc(W, (size_t)n_pad * od);
        ev.st_noise = dalloc(W, (size_t)n_pad * ad);
        ev.st_out = dalloc(W, (size_t)n_pad * ad);
        ev.p_os = make_pass(W, NET_BC, n_pad, ev.X, false, false);
        emit_lane = 0;
        emit_forward(ev.prog_os, ev.p_os, false);
        schedule(ev.prog_os, W);
    }
    // FQL, IFQL: the one-step actor (prog_os) and the Euler flow of the BC actor (prog_flow); IFQL's critic pair for best-of-N scoring;
    // a visual agent's two encoders
    void build_fql_eval(Eval& ev) {
        auto& W = ev.allocs;
        const int od = cfg.obs_dim, ad = cfg.act_dim, n_pad = ev.n_pad;
        ev.X = dalloc(W, (size_t)n_pad * nets[NET_OS].in_p());
        ev.Xf = dalloc(W, (size_t)n_pad * nets[NET_BC].in_p());
        ev.tgt = dalloc(W, (size_t)n_pad * pad16(ad));
        ev.st_obs = dalloc(W, (size_t)n_pad * od);
        ev.st_noise = dalloc(W, (size_t)n_pad * ad);
        ev.st_out = dalloc(W, (size_t)n_pad * ad);
        ev.p_os = make_pass(W, NET_OS, n_pad, ev.X, false, false);
        ev.p_eu = make_pass(W, NET_BC, n_pad, ev.Xf, false, false);
        emit_lane = 0;
        emit_forward(ev.prog_os, ev.p_os, false, GF_CLIP_OUT);
        const int fs = cfg.flow_steps;
        for (int s = 0; s < fs; ++s)
            emit_forward(ev.prog_flow, ev.p_eu, false, GF_EULER | (s == fs - 1 ? GF_EULER_LAST : 0), ev.Xf, ev.tgt,
                         1.0f / (float)fs, (float)(s + 1) / (float)fs);
        schedule(ev.prog_os, W);
        schedule(ev.prog_flow, W);
        if (desc().sampler == SMP_BEST_OF_N) {   // the scoring pass: the critic pair on every sample row
            ev.Xq = dalloc(W, (size_t)n_pad * nets[NET_C0].in_p());
            for (int e = 0; e < 2; ++e) {
                ev.p_q[e] = make_pass(W, NET_C0 + e, n_pad, ev.Xq, false, false);
                emit_forward(ev.prog_q, ev.p_q[e], false);
            }
            schedule(ev.prog_q, W);
        }
        if (visual) {
            const size_t ib = (size_t)cfg.img_h * cfg.img_w * cfg.img_c;
            ev.st_img = (unsigned char*)dalloc(W, ((size_t)n_pad * ib + 3) / 4 + 4);
            ev.eb_os = make_enc_buf(W, ENC_OS, n_pad, ev.st_img, false);
            ev.eb_bc = make_enc_buf(W, ENC_BC, n_pad, ev.st_img, false);
            emit_lane = 1;   // throughput kernels (the encoder's Dense has K = flat > 1024)
            emit_encoder_forward(ev.prog_enc_os, ev.eb_os);
            emit_encoder_forward(ev.prog_enc_bc, ev.eb_bc);
            emit_lane = 0;
            schedule(ev.prog_enc_os, W);
            schedule(ev.prog_enc_bc, W);
        }
    }
    // The workspace of a sampling call over n_pad padded rows.  sweep: the CFG kinds' program with one guidance weight per row, a workspace
    // of its own under its own key, so that no sample_actions workspace or program changes and neither call is ever handed the other's.
    Eval& get_eval(int n_pad, bool sweep = false) {
        const std::pair<int, bool> key{n_pad, sweep};
        auto it = evals.find(key);
        if (it != evals.end()) return *it->second;
        auto ev = std::make_unique<Eval>();
        ev->n_pad = n_pad;
        switch (desc().sampler) {
            case SMP_FLOW: build_flow_sampler(*ev, flow_shape(sweep)); break;
            case SMP_ACTOR: build_actor_eval(*ev); break;
            case SMP_ONESTEP: case SMP_BEST_OF_N: build_fql_eval(*ev); break;
        }
        return *(evals[key] = std::move(ev));
    }
    // The row-chunk loop of every sampling path.  A chunk is <= 4096 rows (256 image rows) of rows_per_obs rows per observation: its
    // observations and noise are staged, `body` enqueues what differs between the paths - the assemble launch, the program(s) and the
    // finishing launch that writes the chunk's [m, act] actions to c.out - and the actions are copied out or, on the engine's own stream, waited for.
    struct SampleSpec { float temperature = 0.f; int rows_per_obs = 1; bool need_noise = false; int enc = ENC_OS; int noise_rows = -1; bool sweep = false; };   // enc: the encoder of a visual agent's rows; noise_rows: noise rows per observation (-1: rows_per_obs); sweep: the chunk's workspace is the sweep program's (get_eval)
    struct SampleChunk { Eval& ev; const float *o, *z; float* out; int start, m; };   // observations [start, start + m) of the call
    template <typename Body>
    void sample_chunks(const float* obs, const float* noise, int n, float* out, hipStream_t s, bool own_stream, const SampleSpec& sp, Body&& body) {
        if (n <= 0) invalid("n must be positive (got %d)", n);
        if (!obs || !out) invalid("observations/out must not be NULL");
        if (sp.need_noise && !noise) invalid("noises must not be NULL");
        if (!(sp.temperature >= 0.0f)) invalid("temperature must be >= 0");
        const int od = cfg.obs_dim, ad = cfg.act_dim, N = sp.rows_per_obs, NZ = sp.noise_rows >= 0 ? sp.noise_rows : N;
        const int per = std::max(1, (visual ? 256 : 4096) / N);
        for (int start = 0; start < n; start += per) {
            const int m = std::min(per, n - start);
            // (the CFG kinds: N = 2 halves of pad16(m) rows each, so that either half starts on a 16-row tile)
            Eval& ev = get_eval(visual ? (m + 63) & ~63 : flow_sampler() ? N * pad16(m) : pad16(m * N), sp.sweep);
            const float* o;
            if (visual) {   // `obs` is uint8 [n, H, W, C]: encode with the module's encoder, then proceed on the encodings
                const size_t ib = (size_t)cfg.img_h * cfg.img_w * cfg.img_c;
                const unsigned char* src = reinterpret_cast<const unsigned char*>(obs) + (size_t)start * ib;
                HIP_CHECK(hipMemcpyAsync(ev.st_img, src, (size_t)m * ib, hipMemcpyDefault, s));
                if (!is_device_ptr(src)) staged_host = true;
                run_launches(sp.enc == ENC_BC ? ev.prog_enc_bc : ev.prog_enc_os, s);
                o = sp.enc == ENC_BC ? ev.eb_bc.E : ev.eb_os.E;
            } else {
                o = stage(obs + (size_t)start * od, ev.st_obs, (size_t)m * od, s);
            }
            const float* z = noise ? stage(noise + (size_t)start * NZ * ad, ev.st_noise, (size_t)m * NZ * ad, s) : nullptr;
            drain_staging(s);
            float* dst = out + (size_t)start * ad;
            const bool dev_out = is_device_ptr(dst);
            body(SampleChunk{ev, o, z, dev_out ? dst : ev.st_out, start, m});
            HIP_CHECK(hipGetLastError());
            if (!dev_out) {
                HIP_CHECK(hipMemcpyAsync(dst, ev.st_out, (size_t)m * ad * sizeof(float), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
            } else if (own_stream) {
                // device output on the engine's private stream: the caller has no handle to order its reads against, so finish here
                HIP_CHECK(hipStreamSynchronize(s));
            }
        }
    }
    // FQL: the one-step actor, or (flow) the Euler flow of the BC actor on the caller's noises.  A seeded draw is keyed per chunk (sd + start).
    void eval_rows(bool flow, const float* obs, const float* noise, uint64_t sd, int n, float* out, hipStream_t s, bool own_stream = false) {
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        sample_chunks(obs, noise, n, out, s, own_stream, SampleSpec{0.f, 1, flow, flow ? ENC_BC : ENC_OS}, [&](const SampleChunk& c) {
            AssembleArgs a{c.o, c.z, flow ? c.ev.Xf : c.ev.X, seed, sd + (uint64_t)c.start, c.m, c.ev.n_pad, od, ad,
                           flow ? nets[NET_BC].in_p() : nets[NET_OS].in_p()};
            hipLaunchKernelGGL(fql_assemble_kernel, dim3((c.ev.n_pad + 3) / 4), dim3(FQL_THREADS), 0, s, a);
            run_launches(flow ? c.ev.prog_flow : c.ev.prog_os, s);
            const float* src16 = flow ? c.ev.tgt : c.ev.p_os.out;
            hipLaunchKernelGGL(fql_extract_kernel, dim3((c.m * ad + 255) / 256), dim3(256), 0, s, src16, c.out, c.m, ad, pad16(ad));
        });
    }
    // The actors on obs: the actor's forward over the rows, then the kind's own launch on its output (KindDesc::act).  noise: [n, act] raw
    // N(0, 1) or null (Philox keyed by (seed, sd) and the row number of the call: chunking does not change the draw).
    void sample_actor(const float* obs, const float* noise, uint64_t sd, float temperature, int n, float* out, hipStream_t s, bool own_stream) {
        const int od = cfg.obs_dim;
        sample_chunks(obs, noise, n, out, s, own_stream, SampleSpec{temperature}, [&](const SampleChunk& c) {
            AssembleArgs aa{c.o, nullptr, c.ev.X, seed, sd, c.m, c.ev.n_pad, od, 0, nets[NET_BC].in_p()};   // [obs | 0]
            hipLaunchKernelGGL(fql_assemble_kernel, dim3((c.ev.n_pad + 3) / 4), dim3(FQL_THREADS), 0, s, aa);
            run_launches(c.ev.prog_os, s);
            desc().act(*this, ActChunk{c.ev.p_os.out, c.z, c.out, sd, c.m, c.start, temperature}, s);
        });
    }
    // sample_actions of the flow policies (build_flow_sampler's program between the kind's assemble launch and the extract launch):
    //   BC (agents/bc.py:86-101): x ~ N(0, I); S times x += policy(obs, x, i / S) / S; clip
    //   IQL-diffusion (agents/iql_diffusion.py:249-270): ... S times v = v_unc + cfg (v_pos - v_unc), x += v / S; clip
    //   CFGRL (agents/cfgrl.py:70-100): ... flow_steps times v = v_unc + cfg (v_cond - v_unc), x += v / flow_steps; clip.  goals: [n, G]
    // The CFG kinds run 2n rows per call, [pos ; unc], in chunks of 2048 observations.  Rows are independent (16-row tiles and per-element
    // kernels, the same at every n), so row j of a call equals the single-observation call on the same noise.  noise: [n, act] or null
    // (Philox keyed by (seed, sd) and the row number of the call: chunking does not change the draw).
    // sweep (fql_iqld_sample_actions_cfgs, fql_cfgrl_sample_actions_cfgs): one guidance weight per row, the sweep program on the same
    // assemble and extract launches.  Row j equals the scalar call on row j with cfg = cfgs[j], bit for bit.  cfgs: [n], host (checked
    // here: finite) or device (not read on the host); each chunk's weights are copied into the workspace buffer the program was bound to,
    // with 0 behind them.
    struct FlowCall { const float* goals = nullptr; float cfg = 1.0f; const float* cfgs = nullptr; bool sweep = false; };
    void sample_flow(const float* obs, const float* noise, uint64_t sd, int n, float* out, hipStream_t s, bool own_stream, const FlowCall& fc) {
        const FlowShape sh = flow_shape(fc.sweep);
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad), Gd = sh.goal_dim, inp = nets[NET_BC].in_p();
        if (fc.sweep) {
            if (n <= 0) invalid("n must be positive (got %d)", n);
            if (!fc.cfgs) invalid("cfgs must not be NULL (one guidance weight per row)");
        }
        if (Gd && !fc.goals) invalid("goals must not be NULL (the conditional pass reads them: agents/cfgrl.py:93)");
        const bool host_cfgs = fc.sweep && !is_device_ptr(fc.cfgs);
        if (host_cfgs)
            for (int i = 0; i < n; ++i)
                if (!std::isfinite(fc.cfgs[i])) invalid("cfgs[%d] = %g: every guidance weight must be finite", i, (double)fc.cfgs[i]);
        if (sh.halves == 2 && !fc.sweep) {
            if (!std::isfinite(fc.cfg)) invalid("cfg must be finite");
            sample_cfg = fc.cfg;
        }
        SampleSpec sp{};
        sp.rows_per_obs = sh.halves; sp.noise_rows = 1; sp.sweep = fc.sweep;
        sample_chunks(obs, noise, n, out, s, own_stream, sp, [&](const SampleChunk& c) {
            Eval& ev = c.ev;
            const int half = ev.n_pad / sh.halves;
            if (fc.sweep) {
                HIP_CHECK(hipMemcpyAsync(ev.cfgs, fc.cfgs + c.start, (size_t)c.m * sizeof(float), hipMemcpyDefault, s));
                if (host_cfgs) staged_host = true;
                if (half > c.m) HIP_CHECK(hipMemsetAsync(ev.cfgs + c.m, 0, (size_t)(half - c.m) * sizeof(float), s));
            }
            const float* g = Gd ? stage(fc.goals + (size_t)c.start * Gd, ev.st_goal, (size_t)c.m * Gd, s) : nullptr;
            drain_staging(s);
            if (Gd) {
                CfgrlAssembleArgs aa{c.o, g, P + emb_off, c.z, ev.X, ev.Xf, seed, sd, c.m, half, od, Gd, ad, inp, ap, c.start};
                hipLaunchKernelGGL(fql_cfgrl_assemble_kernel, dim3((half + 3) / 4), dim3(FQL_THREADS), 0, s, aa);
            } else {   // BC over its n_pad rows, IQL-diffusion over the half the two passes share
                BcAssembleArgs aa{c.o, c.z, ev.X, ev.Xf, seed, sd, c.m, half, od, ad, inp, ap, c.start};
                hipLaunchKernelGGL(fql_bc_assemble_kernel, dim3((half + 3) / 4), dim3(FQL_THREADS), 0, s, aa);
            }
            run_launches(ev.prog_flow, s);
            hipLaunchKernelGGL(fql_extract_kernel, dim3((c.m * ad + 255) / 256), dim3(256), 0, s, (const float*)ev.tgt, c.out, c.m, ad, ap);
        });
    }
    // launches of one flow-sampling call on a single chunk, counted from the built program: assemble, the program's launches, extract.
    // The smallest workspace of the kind (the count does not depend on the rows): 16 rows, or two halves of 16.
    int64_t sample_flow_launches(bool sweep) { return 2 + (int64_t)get_eval(flow_shape(sweep).halves * 16, sweep).prog_flow.launches.size(); }
    // IFQL sample_actions (agents/ifql.py:123-155), per observation: num_samples noises through the Euler flow of actor_flow, clip, score by
    // min(q1, q2) of the critic, keep the first argmax.  [n, od] is a batched extension of the reference's single observation: row by row
    // equal to n calls with the same noises.  Chunks of <= 4096 sample rows.
    void sample_best_of_n(const float* obs, const float* noise, uint64_t sd, int n, float* out, hipStream_t s, bool own_stream) {
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad), N = num_samples;
        sample_chunks(obs, noise, n, out, s, own_stream, SampleSpec{0.f, N}, [&](const SampleChunk& c) {
            Eval& ev = c.ev;
            IfqlRepeatArgs ra{c.o, c.z, ev.Xf, seed, sd, c.m, N, ev.n_pad, od, ad, nets[NET_BC].in_p(), c.start * N};
            hipLaunchKernelGGL(fql_ifql_repeat_kernel, dim3((ev.n_pad + 3) / 4), dim3(FQL_THREADS), 0, s, ra);
            run_launches(ev.prog_flow, s);
            IfqlQinArgs qa{c.o, ev.tgt, ev.Xq, c.m, N, ev.n_pad, od, ad, ap, nets[NET_C0].in_p()};
            hipLaunchKernelGGL(fql_ifql_qin_kernel, dim3((ev.n_pad + 3) / 4), dim3(FQL_THREADS), 0, s, qa);
            run_launches(ev.prog_q, s);
            IfqlSelectArgs sa{ev.p_q[0].out, ev.p_q[1].out, ev.tgt, c.out, c.m, N, ad, ap};
            hipLaunchKernelGGL(fql_ifql_select_kernel, dim3((c.m + 3) / 4), dim3(FQL_THREADS), 0, s, sa);
        });
    }
    // sample_actions of the handle's kind (the temperature is ReBRAC's, SAC's and IQL's)
    void sample(const float* obs, const float* noise, uint64_t sd, float temperature, int n, float* out, hipStream_t s, bool own_stream) {
        switch (desc().sampler) {
            case SMP_ONESTEP: eval_rows(false, obs, noise, sd, n, out, s, own_stream); break;
            case SMP_BEST_OF_N: sample_best_of_n(obs, noise, sd, n, out, s, own_stream); break;
            case SMP_FLOW: sample_flow(obs, noise, sd, n, out, s, own_stream, FlowCall{}); break;   // (BC: the CFG kinds' calls pass their cfg and goals to sample_flow)
            case SMP_ACTOR: sample_actor(obs, noise, sd, temperature, n, out, s, own_stream); break;
        }
    }
    // ---------------------------------------------------------------------------------------
    // module queries: agent.network.select(module)(...) (utils/flax_utils.py ModuleDict / TrainState.select), DESIGN.md section 21
    // ---------------------------------------------------------------------------------------
    // The modules a handle of this kind answers for (the row's ModuleSpec list).
    // Not there, and why (include/fql_amd.h): the Gaussian actors return a distribution object in the reference; IQL-diffusion's actor, BC's
    // policy and CFGRL's actor_flow read host-built embeddings and the unc_embed row.
    std::vector<ModuleSpec> modules() const { return {desc().modules, desc().modules + desc().nmodules}; }
    // The workspace of module `mi` over n_pad rows: the padded input, one pass per member on lane 0 (the 16-row kernels of every sampling
    // path: a row's result does not depend on the rows beside it) without saved activations, scheduled once.
    Query& get_query(int mi, const ModuleSpec& sp, int n_pad) {
        const std::pair<int, int> key{mi, n_pad};
        auto it = queries.find(key);
        if (it != queries.end()) return *it->second;
        auto q = std::make_unique<Query>();
        auto& W = q->allocs;
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        q->X = dalloc(W, (size_t)n_pad * nets[sp.net].in_p());
        q->st_obs = dalloc(W, (size_t)n_pad * od);
        if (sp.act) q->st_act = dalloc(W, (size_t)n_pad * ad);
        if (sp.times) q->st_t = dalloc(W, (size_t)n_pad);
        q->st_out = dalloc(W, (size_t)n_pad * (sp.scalar ? sp.members : ad));
        emit_lane = 0;
        for (int e = 0; e < sp.members; ++e) {
            q->p[e] = make_pass(W, sp.net + e, n_pad, q->X, false, false);
            emit_forward(q->prog, q->p[e], false);
        }
        schedule(q->prog, W);
        return *(queries[key] = std::move(q));
    }
    // One module's forward on the caller's rows, in chunks of <= 4096 as the samplers': stage, assemble [obs | act | t], the program, then
    // the heads [members, n] (member-major at the chunk's offset) or the [m, act] rows.  A host result leaves through the staging buffer.
    void module_forward(int mi, const ModuleSpec& sp, const float* obs, const float* act, const float* times, int n, float* out,
                        hipStream_t s, bool own_stream) {
        if (n <= 0) invalid("n must be positive (got %d)", n);
        if (!obs || !out) invalid("observations/out must not be NULL");
        if (sp.act && !act) invalid("module '%s' takes actions: actions must not be NULL", sp.name);
        if (!sp.act && act) invalid("module '%s' takes observations only: actions must be NULL", sp.name);
        if (sp.times && !times) invalid("module '%s' takes times: times must not be NULL", sp.name);
        if (!sp.times && times) invalid("module '%s' takes no times: times must be NULL", sp.name);
        const int od = cfg.obs_dim, ad = cfg.act_dim, ap = pad16(ad);
        const bool dev_out = is_device_ptr(out);
        for (int start = 0; start < n; start += 4096) {
            const int m = std::min(4096, n - start), n_pad = pad16(m);
            Query& q = get_query(mi, sp, n_pad);
            const float* o = stage(obs + (size_t)start * od, q.st_obs, (size_t)m * od, s);
            const float* a = act ? stage(act + (size_t)start * ad, q.st_act, (size_t)m * ad, s) : nullptr;
            const float* t = times ? stage(times + start, q.st_t, (size_t)m, s) : nullptr;
            drain_staging(s);
            const QueryAssembleArgs aa{o, a, t, q.X, m, n_pad, od, ad, nets[sp.net].in_p()};
            hipLaunchKernelGGL(fql_query_assemble_kernel, dim3((n_pad + 3) / 4), dim3(FQL_THREADS), 0, s, aa);
            run_launches(q.prog, s);
            if (sp.scalar) {
                const QueryHeadsArgs ha{{q.p[0].out, sp.members == 2 ? q.p[1].out : nullptr}, dev_out ? out + start : q.st_out, m, sp.members,
                                        dev_out ? (size_t)n : (size_t)m};
                hipLaunchKernelGGL(fql_query_heads_kernel, dim3((m * sp.members + FQL_THREADS - 1) / FQL_THREADS), dim3(FQL_THREADS), 0, s, ha);
            } else {
                hipLaunchKernelGGL(fql_extract_kernel, dim3((m * ad + 255) / 256), dim3(256), 0, s, (const float*)q.p[0].out,
                                   dev_out ? out + (size_t)start * ad : q.st_out, m, ad, ap);
            }
            HIP_CHECK(hipGetLastError());
            if (!dev_out) {
                if (sp.scalar)
                    for (int e = 0; e < sp.members; ++e)
                        HIP_CHECK(hipMemcpyAsync(out + (size_t)e * n + start, q.st_out + (size_t)e * m, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, s));
                else
                    HIP_CHECK(hipMemcpyAsync(out + (size_t)start * ad, q.st_out, (size_t)m * ad * sizeof(float), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
            } else if (own_stream) {
                HIP_CHECK(hipStreamSynchronize(s));   // a device result on the engine's private stream: finished before return, as the samplers'
            }
        }
    }
    // ReBRAC host batches: the FQL ones plus next_actions [B, act] (source_from_dataset takes the dataset's actions one row on)
    void rebrac_source_from_batch(const float* obs, const float* act, const float* rew, const float* mask, const float* nobs, const float* nact,
                                  int batch, const fql_noise* nz, int advance, hipStream_t s) {
        if (batch != B) invalid("batch_size %d does not match the engine's workspace (%d); call fql_set_batch_size", batch, B);
        if (!obs || !act || !rew || !mask || !nobs || !nact) invalid("batch pointers must not be NULL (ReBRAC batches carry next_actions)");
        const int od = cfg.obs_dim, ad = cfg.act_dim;
        SrcDesc d{};
        d.obs = stage(obs, in_obs, (size_t)B * od, s);
        d.nobs = stage(nobs, in_nobs, (size_t)B * od, s);
        d.act = stage(act, in_act, (size_t)B * ad, s);
        d.rew = stage(rew, in_rew, B, s);
        d.mask = stage(mask, in_mask, B, s);
        d.nact = stage(nact, in_nact, (size_t)B * ad, s);
        fill_noise(d, nz, s);
        d.advance = advance;
        drain_staging(s);
        set_source(d, s);
    }
};

// ================================================================================================
// k_kinds: one row per kind (KindDesc, above), each kind's hooks in front of the table
// ================================================================================================
namespace {

// ---- FQL (agents/fql.py) ----
const Mod k_fql_mods[4] = {{"modules_actor_bc_flow", "mlp", NET_BC, -1, true, ENC_BC},
                           {"modules_actor_onestep_flow", "mlp", NET_OS, -1, true, ENC_OS},
                           {"modules_critic", "value_net", NET_C0, NET_C1, true, ENC_C},
                           {"modules_target_critic", "value_net", NET_T0, NET_T1, false, ENC_T}};
const ModuleSpec k_fql_modules[4] = {{"critic", NET_C0, 2, true, true, false}, {"target_critic", NET_T0, 2, true, true, false},
                                     {"actor_bc_flow", NET_BC, 1, false, true, true}, {"actor_onestep_flow", NET_OS, 1, false, true, false}};
// the kinds with a value net answer for the first three of these, IFQL for its actor_flow too; the other critic kinds for the pair alone
const ModuleSpec k_value_modules[4] = {{"critic", NET_C0, 2, true, true, false}, {"target_critic", NET_T0, 2, true, true, false},
                                       {"value", NET_OS, 1, true, false, false}, {"actor_flow", NET_BC, 1, false, true, true}};
void fql_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.actor_net(od + ad + 1, ad); e.nets[NET_OS] = e.actor_net(od + ad, ad); }

// ---- IFQL (agents/ifql.py:215-225): the value net is a 1-member Value, so its leaves are unstacked ----
const Mod k_ifql_mods[4] = {{"modules_actor_flow", "mlp", NET_BC, -1, true, ENC_BC},
                            {"modules_critic", "value_net", NET_C0, NET_C1, true, ENC_C},
                            {"modules_target_critic", "value_net", NET_T0, NET_T1, false, ENC_T},
                            {"modules_value", "value_net", NET_OS, -1, true, ENC_OS}};
void ifql_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.actor_net(od + ad + 1, ad); e.nets[NET_OS] = e.value_net(od); }   // value (agents/ifql.py:188-193)
const char* ifql_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_ifql_config*>(kind_cfg);
    if (!(c->expectile > 0.0f && c->expectile < 1.0f)) return "expectile must be in (0, 1)";
    if (c->num_samples < 1 || c->num_samples > 4096) return "num_samples must be in [1, 4096]";
    return nullptr;
}
void ifql_adopt(fql_engine& e, const void* kind_cfg) {
    const auto* c = static_cast<const fql_ifql_config*>(kind_cfg);
    e.expectile = c->expectile; e.num_samples = c->num_samples;
}

// ---- ReBRAC (agents/rebrac.py:199-213): Actor modules hold actor_net/Dense_0..nh-1 (+ LayerNorm_i) and mean_net (the last layer) ----
const Mod k_rebrac_mods[4] = {{"modules_actor", "actor_net", NET_BC, -1, true, ENC_BC, true},
                              {"modules_critic", "value_net", NET_C0, NET_C1, true, ENC_C},
                              {"modules_target_actor", "actor_net", NET_TA, -1, false, ENC_BC, true},
                              {"modules_target_critic", "value_net", NET_T0, NET_T1, false, ENC_T}};
void rebrac_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.nets[NET_TA] = e.actor_net(od, ad); }   // actor (utils/networks.py:82-150)
const char* rebrac_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_rebrac_config*>(kind_cfg);
    if (!(c->actor_noise >= 0.0f) || !(c->actor_noise_clip >= 0.0f)) return "actor_noise and actor_noise_clip must be >= 0";
    if (!(c->actor_fc_scale > 0.0f)) return "actor_fc_scale must be > 0";
    if (!std::isfinite(c->alpha_actor) || !std::isfinite(c->alpha_critic)) return "alpha_actor and alpha_critic must be finite";
    if (c->tanh_squash != 0 && c->tanh_squash != 1) return "tanh_squash must be 0 or 1";
    return nullptr;
}
void rebrac_adopt(fql_engine& e, const void* kind_cfg) { e.rcfg = *static_cast<const fql_rebrac_config*>(kind_cfg); }
// agents/rebrac.py:136-152: clip(mode(actor(obs)) + clip(N(0, 1) actor_noise temperature, +-actor_noise_clip), -1, 1)
void rebrac_act(const fql_engine& e, const ActChunk& c, hipStream_t s) {
    const int ad = e.cfg.act_dim, ap = pad16(ad);
    RebracActArgs ra{c.mean, c.z, c.out, e.seed, c.sd, c.m, ad, ap, ad, ad, 0, c.start, c.z ? 1 : 2, e.rcfg.tanh_squash, 1,
                     e.rcfg.actor_noise * c.temperature, e.rcfg.actor_noise_clip};
    hipLaunchKernelGGL(fql_rebrac_act_kernel, dim3((c.m * ad + FQL_THREADS - 1) / FQL_THREADS), dim3(FQL_THREADS), 0, s, ra);
}

// ---- SAC (agents/sac.py:170-196): Actor (actor_net, log_std_net, mean_net), the 0-d LogParam (n0 = -1), critic, target critic ----
const Mod k_sac_mods[4] = {{"modules_actor", "actor_net", NET_BC, -1, true, ENC_BC, true},
                           {"modules_alpha", "", -1, -1, true, ENC_BC},
                           {"modules_critic", "value_net", NET_C0, NET_C1, true, ENC_C},
                           {"modules_target_critic", "value_net", NET_T0, NET_T1, false, ENC_T}};
void sac_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.actor_net(od, 2 * pad16(ad)); }   // actor_net + [mean_net | log_std_net]
const char* sac_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_sac_config*>(kind_cfg);
    if (c->state_dependent_std != 1) return "only state_dependent_std = 1 is available (the const_std=False vector form is not)";
    if (c->tanh_squash != 0 && c->tanh_squash != 1) return "tanh_squash must be 0 or 1";
    if (!(c->actor_fc_scale > 0.0f)) return "actor_fc_scale must be > 0";
    if (!std::isnan(c->target_entropy) && !std::isfinite(c->target_entropy)) return "target_entropy must be finite or NaN (automatic)";
    if (std::isnan(c->target_entropy) && !std::isfinite(c->target_entropy_multiplier)) return "target_entropy_multiplier must be finite";
    return nullptr;
}
void sac_adopt(fql_engine& e, const void* kind_cfg) {   // sac.py create: target_entropy = -target_entropy_multiplier * action_dim when None
    e.scfg = *static_cast<const fql_sac_config*>(kind_cfg);
    e.target_entropy = std::isnan(e.scfg.target_entropy) ? -e.scfg.target_entropy_multiplier * (float)e.cfg.act_dim : e.scfg.target_entropy;
}
bool sac_leaves(fql_engine& e, LeafSite at, const Mod* m) {
    if (at == LS_NO_NET) {   // modules_alpha/log_value: shape (), one float padded to an Adam quad
        e.add_leaf(std::string(m->name) + "/log_value", false, 1, 1, e.alpha_off, 1, 4);
        e.leaves.back().ndim = 0;
        return true;
    }
    if (at != LS_ACTOR_HEAD) return false;
    // the two heads: column blocks [0, ap) and [ap, 2 ap) of the last layer, each read back as [H, act] / [act]
    const Layer& a = e.nets[m->n0].layers.back();
    const int ad = e.cfg.act_dim, ap = pad16(ad);
    for (const char* head : {"log_std_net", "mean_net"}) {
        const size_t c0 = std::strcmp(head, "mean_net") == 0 ? 0 : (size_t)ap;
        const std::string hb = std::string(m->name) + "/" + head + "/";
        e.add_leaf(hb + "bias", false, 1, ad, a.b + c0, 1, ap);
        e.add_leaf(hb + "kernel", true, a.in, ad, a.w + c0, a.in_p, a.out_p);
        e.leaves.back().segs[0].chunk_w = ap;
    }
    return true;
}
// agents/sac.py:125-136: clip(tanh(mean + exp(ls) temperature eps), -1, 1) (no tanh without tanh_squash)
void sac_act(const fql_engine& e, const ActChunk& c, hipStream_t s) {
    const int ad = e.cfg.act_dim, ap = pad16(ad);
    SacActArgs sa{c.mean, c.z, c.out, c.out, nullptr, e.seed, c.sd, c.m, ad, ap, ad, ad, 0, c.start, c.m, c.z ? 1 : 2, e.scfg.tanh_squash, 1, c.temperature};
    hipLaunchKernelGGL(fql_sac_act_kernel, dim3((c.m + FQL_THREADS - 1) / FQL_THREADS), dim3(FQL_THREADS), 0, s, sa);
}

// ---- BC (agents/bc.py:26-44): no modules, the leaves of one bare net, policy(obs, x_t, emb(t)) ----
void bc_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.actor_net(od + ad + BC_EMB, ad); }
const char* bc_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_bc_config*>(kind_cfg);
    return c->denoise_steps < 1 || c->denoise_steps > 1024 ? "denoise_steps must be in [1, 1024]" : nullptr;
}
void bc_adopt(fql_engine& e, const void* kind_cfg) { e.bc_steps = static_cast<const fql_bc_config*>(kind_cfg)->denoise_steps; }

// ---- IQL (agents/iql.py:222-227): Actor (actor_net, log_stds with const_std = 0, mean_net), critic, target critic, the 1-member value ----
const Mod k_iql_mods[4] = {{"modules_actor", "actor_net", NET_BC, -1, true, ENC_BC, true},
                           {"modules_critic", "value_net", NET_C0, NET_C1, true, ENC_C},
                           {"modules_target_critic", "value_net", NET_T0, NET_T1, false, ENC_T},
                           {"modules_value", "value_net", NET_OS, -1, true, ENC_OS}};
void iql_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.actor_net(od, ad); e.nets[NET_OS] = e.value_net(od); }
const char* iql_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_iql_config*>(kind_cfg);
    if (!(c->expectile > 0.0f && c->expectile < 1.0f)) return "expectile must be in (0, 1)";
    if (!std::isfinite(c->alpha)) return "alpha must be finite";
    if (c->actor_loss != 0 && c->actor_loss != 1) return "actor_loss must be 0 (awr) or 1 (ddpgbc)";
    if (c->const_std != 0 && c->const_std != 1) return "const_std must be 0 or 1";
    return nullptr;
}
void iql_adopt(fql_engine& e, const void* kind_cfg) { e.qcfg = *static_cast<const fql_iql_config*>(kind_cfg); }
InfoSet iql_infos(const fql_engine& e) {
    const bool ddpg = e.qcfg.actor_loss == 1;
    return {k_iql_info_names[ddpg ? 1 : 0], ddpg ? FQL_IQL_DDPGBC_NUM_INFO : FQL_IQL_AWR_NUM_INFO};
}
size_t iql_extra(const fql_engine& e) { return e.qcfg.const_std ? 0 : pad16(e.cfg.act_dim); }   // modules_actor/log_stds: [act], padded to ap
bool iql_leaves(fql_engine& e, LeafSite at, const Mod* m) {   // "log_stds" sorts between actor_net and mean_net
    if (at == LS_ACTOR_HEAD && !e.qcfg.const_std)
        e.add_leaf(std::string(m->name) + "/log_stds", false, 1, e.cfg.act_dim, e.ls_off, 1, pad16(e.cfg.act_dim));
    return false;
}
// agents/iql.py:158-169: clip(mean + exp(clip(log_stds)) temperature eps, -1, 1)
void iql_act(const fql_engine& e, const ActChunk& c, hipStream_t s) {
    const int ad = e.cfg.act_dim, ap = pad16(ad);
    IqlSampleArgs sa{c.mean, e.qcfg.const_std ? nullptr : e.P + e.ls_off, c.z, c.out, e.seed, c.sd, c.m, ad, ap, c.start, c.temperature};
    hipLaunchKernelGGL(fql_iql_sample_kernel, dim3((c.m * ad + FQL_THREADS - 1) / FQL_THREADS), dim3(FQL_THREADS), 0, s, sa);
}

// ---- IQL-diffusion (agents/iql_diffusion.py:87-91): four bare TrainStates, no ModuleDict; the actor's leaves are BC's plus the embedding ----
const Mod k_iqld_mods[3] = {{"critic", "value_net", NET_C0, NET_C1, true, ENC_C},
                            {"target_critic", "value_net", NET_T0, NET_T1, false, ENC_T},
                            {"value", "value_net", NET_OS, -1, true, ENC_OS}};
void iqld_nets(fql_engine& e, int od, int ad) {   // iql_diffusion.py:54-67
    e.nets[NET_BC] = e.actor_net(od + ad + BC_EMB + IQLD_EMBED, ad); e.nets[NET_OS] = e.value_net(od);
}
const char* iqld_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_iqld_config*>(kind_cfg);
    if (c->optimal_var == 3 || c->optimal_var == 4)
        return "optimal_var 'softmax' / 'sampled_adv_softmax' (the continuous policy with an external bc_agent) is not available: "
               "the binary family only (0 binary, 1 binary_awr_loss, 2 binary_softmax_loss)";
    if (c->optimal_var < 0 || c->optimal_var > 4) return "optimal_var must be 0 (binary), 1 (binary_awr_loss) or 2 (binary_softmax_loss)";
    if (c->opt_decay_schedule != 0) return "opt_decay_schedule 'cosine' is not available (a constant actor_lr only)";
    if (!(c->expectile > 0.0f && c->expectile < 1.0f)) return "expectile must be in (0, 1)";
    if (!(c->actor_lr > 0.0f) || !(c->value_lr > 0.0f) || !(c->critic_lr > 0.0f)) return "actor_lr, value_lr and critic_lr must be > 0";
    if (!std::isfinite(c->awr_temperature) || !std::isfinite(c->softmax_beta)) return "awr_temperature and softmax_beta must be finite";
    if (c->target_extraction != 0 && c->target_extraction != 1) return "target_extraction must be 0 or 1";
    if (c->denoise_steps < 1 || c->denoise_steps > 1024) return "denoise_steps must be in [1, 1024]";
    return nullptr;
}
void iqld_adopt(fql_engine& e, const void* kind_cfg) { e.dcfg = *static_cast<const fql_iqld_config*>(kind_cfg); e.bc_steps = e.dcfg.denoise_steps; }
bool iqld_leaves(fql_engine& e, LeafSite at, const Mod*) {   // nn.Embed(2, 32): sorts behind Dense_0
    if (at == LS_BARE_HEAD) e.add_leaf("actor/Embed_0/embedding", true, 2, IQLD_EMBED, e.emb_off, 2, IQLD_EMBED);
    return false;
}
// nn.Embed(2, 32): with in_axis = -2 and out_axis = 0 both name axis 0: in_size = out_size = 2, receptive field = 64 / (2 * 2) = 16,
// fan_in = 2 * 16 = 32 (the feature count)
EmbedInit iqld_embed_init(const fql_engine&) { return {2 * IQLD_EMBED, IQLD_EMBED}; }

// ---- CFGRL (agents/cfgrl.py:143-156): one ModuleDict, actor_flow and the [1, G] embedding behind it ----
const Mod k_cfgrl_mods[1] = {{"modules_actor_flow", "mlp", NET_BC, -1, true, ENC_BC}};
void cfgrl_nets(fql_engine& e, int od, int ad) { e.nets[NET_BC] = e.actor_net(od + e.gcfg.goal_dim + ad + 1, ad); }   // actor_flow(obs, goals, x_t, t) (utils/networks.py:237-284)
const char* cfgrl_check(const void* kind_cfg) {
    const auto* c = static_cast<const fql_cfgrl_config*>(kind_cfg);
    if (c->actor_geom_sample != 0)
        return "actor_geom_sample = True is not available: the geometric offset is a ceil of a ratio of logarithms, which the device's "
               "log and numpy's may round to different integers (uniform trajectory goals only)";
    if (c->goal_dim < 1 || c->goal_dim > 1024) return "goal_dim must be in [1, 1024] (layer 0 is obs + goal_dim + act + 1 wide)";
    if (c->flow_steps < 1 || c->flow_steps > 1024) return "flow_steps must be in [1, 1024]";
    if (!std::isfinite(c->cfg)) return "cfg must be finite";
    if (!(c->p_uncond >= 0.0 && c->p_uncond <= 1.0)) return "p_uncond must be in [0, 1]";
    const double pc = c->actor_p_curgoal, pt = c->actor_p_trajgoal, pr = c->actor_p_randomgoal;
    if (!(pc >= 0.0 && pt >= 0.0 && pr >= 0.0) || std::fabs(pc + pt + pr - 1.0) > 1e-8)   // utils/datasets.py:159-161
        return "actor_p_curgoal + actor_p_trajgoal + actor_p_randomgoal must be 1, each >= 0";
    return nullptr;
}
void cfgrl_adopt(fql_engine& e, const void* kind_cfg) { e.gcfg = *static_cast<const fql_cfgrl_config*>(kind_cfg); }
bool cfgrl_leaves(fql_engine& e, LeafSite at, const Mod*) {   // nn.Embed(1, goal_dim): "modules_unc_embed" sorts behind "modules_actor_flow"
    if (at == LS_LAST) e.add_leaf("modules_unc_embed/Embed_0/embedding", true, 1, e.gcfg.goal_dim, e.emb_off, 1, pad16(e.gcfg.goal_dim));
    return false;
}
// nn.Embed(1, G): by the derivation at iqld_embed_init in_size = out_size = 1, receptive field = G, fan_in = G
EmbedInit cfgrl_embed_init(const fql_engine& e) { return {e.gcfg.goal_dim, e.gcfg.goal_dim}; }

const KindDesc k_kinds[kNumKinds] = {
    {"FQL", "an FQL handle", "fql_create", K_CRITIC | K_CHAIN | K_VISUAL,
     k_info_names, FQL_NUM_INFO, nullptr, 10, {0, 4, -1},
     NZ_EPS1 | NZ_X0 | NZ_T | NZ_Z | NZ_EPS2, nullptr,
     nullptr, nullptr, fql_nets, nullptr, nullptr,
     k_fql_mods, 4, nullptr, {"modules_actor_bc_flow/", "modules_actor_onestep_flow/", "modules_critic/"}, nullptr,
     HI_GLOROT, nullptr, nullptr,
     &fql_engine::build_fql_workspace, [](const fql_engine& e) { return e.fql_macs(); },
     SMP_ONESTEP, nullptr, {}, k_fql_modules, 4},
    {"IFQL", "an IFQL handle", "fql_ifql_create", K_CRITIC,
     k_ifql_info_names, FQL_IFQL_NUM_INFO, nullptr, 9, {0, 4, 8},   // agents/ifql.py:79-98: value + critic + actor; nine infos
     NZ_X0 | NZ_T, "IFQL reads only x0 and t of fql_noise (eps1, z and eps2 must be NULL)",
     ifql_check, ifql_adopt, ifql_nets, nullptr, nullptr,
     k_ifql_mods, 4, nullptr, {"modules_actor_flow/", "modules_value/", "modules_critic/"}, nullptr,
     HI_GLOROT, nullptr, nullptr,
     &fql_engine::build_ifql_workspace, [](const fql_engine& e) { return e.ifql_macs(); },
     SMP_BEST_OF_N, nullptr, {}, k_value_modules, 4},
    {"ReBRAC", "a ReBRAC handle", "fql_rebrac_create", K_CRITIC | K_POLYAK_ALL | K_NEXT_ACTIONS,
     k_rebrac_info_names, FQL_REBRAC_NUM_INFO, nullptr, 0, {-1, -1, -1},
     NZ_EPS1, "ReBRAC reads only eps1 of fql_noise (x0, t, z and eps2 must be NULL)",
     rebrac_check, rebrac_adopt, rebrac_nets, nullptr, nullptr,
     k_rebrac_mods, 4, nullptr, {"modules_actor/", "modules_critic/", "modules_critic/"}, nullptr,   // (two trained modules: the critic's range twice)
     HI_GLOROT, [](const fql_engine& e) { return (double)e.rcfg.actor_fc_scale; }, nullptr,
     &fql_engine::build_rebrac_workspace, [](const fql_engine& e) { return e.rebrac_macs(true); },
     SMP_ACTOR, rebrac_act, {}, k_value_modules, 2},
    {"SAC", "a SAC handle", "fql_sac_create", K_CRITIC,
     k_sac_info_names, FQL_SAC_NUM_INFO, nullptr, 0, {-1, -1, -1},
     NZ_EPS1 | NZ_EPS2, "SAC reads only eps1 and eps2 of fql_noise (x0, t and z must be NULL)",
     sac_check, sac_adopt, sac_nets, &fql_engine::alpha_off, [](const fql_engine&) { return (size_t)4; },   // modules_alpha/log_value: one float, padded to an Adam quad
     k_sac_mods, 4, nullptr, {"modules_actor/", "modules_alpha/", "modules_critic/"}, sac_leaves,
     HI_TWO_HEADS, [](const fql_engine& e) { return (double)e.scfg.actor_fc_scale; }, nullptr,
     &fql_engine::build_sac_workspace, [](const fql_engine& e) { return e.sac_macs(); },
     SMP_ACTOR, sac_act, {}, k_value_modules, 2},
    {"BC", "a BC handle", "fql_bc_create", K_TIME_TABLE,
     k_bc_info_names, FQL_BC_NUM_INFO, nullptr, 0, {-1, -1, -1},
     NZ_X0 | NZ_T, "BC reads only x0 and t of fql_noise (eps1, z and eps2 must be NULL)",
     bc_check, bc_adopt, bc_nets, nullptr, nullptr,
     nullptr, 0, "", {nullptr, nullptr, nullptr}, nullptr,   // (one module: every chunk)
     HI_LECUN_TRUNC, nullptr, nullptr,
     &fql_engine::build_bc_workspace, [](const fql_engine& e) { return e.bc_macs(); },
     SMP_FLOW, nullptr, {1, true, 1}, nullptr, 0},
    {"IQL", "an IQL handle", "fql_iql_create", K_CRITIC | K_OWN_INFO,
     nullptr, 0, iql_infos, 0, {-1, -1, -1},
     NZ_EPS1, "IQL reads only eps1 of fql_noise (x0, t, z and eps2 must be NULL)",
     iql_check, iql_adopt, iql_nets, &fql_engine::ls_off, iql_extra,
     k_iql_mods, 4, nullptr, {"modules_actor/", "modules_value/", "modules_critic/"}, iql_leaves,
     HI_GLOROT, [](const fql_engine&) { return 1e-2; }, nullptr,   // Actor.final_fc_init_scale (utils/networks.py:106)
     &fql_engine::build_iql_workspace, [](const fql_engine& e) { return e.iql_macs(); },
     SMP_ACTOR, iql_act, {}, k_value_modules, 3},
    {"IQL-diffusion", "an IQL-diffusion handle", "fql_iqld_create", K_CRITIC | K_OWN_INFO | K_TIME_TABLE | K_ACTOR_STATE,
     k_iqld_info_names, FQL_IQLD_NUM_INFO, nullptr, 0, {-1, -1, -1},
     NZ_X0 | NZ_T, "IQL-diffusion reads only x0 and t of fql_noise (eps1, z and eps2 must be NULL)",
     iqld_check, iqld_adopt, iqld_nets, &fql_engine::emb_off, [](const fql_engine&) { return (size_t)2 * IQLD_EMBED; },   // actor/Embed_0/embedding: [2, 32]
     k_iqld_mods, 3, "actor/", {"actor/", "value/", "critic/"}, iqld_leaves,   // (bare: the policy net is the `actor` field)
     HI_LECUN_TRUNC, nullptr, iqld_embed_init,
     &fql_engine::build_iqld_workspace, [](const fql_engine& e) { return e.iqld_macs(true, true); },
     SMP_FLOW, nullptr, {2, true, 2}, k_value_modules, 3},
    {"CFGRL", "a CFGRL handle", "fql_cfgrl_create", K_GOALS,
     k_cfgrl_info_names, FQL_CFGRL_NUM_INFO, nullptr, 0, {-1, -1, -1},
     NZ_X0 | NZ_T, "CFGRL reads only x0 and t of fql_noise (eps1, z and eps2 must be NULL)",
     cfgrl_check, cfgrl_adopt, cfgrl_nets, &fql_engine::emb_off, [](const fql_engine& e) { return (size_t)pad16(e.gcfg.goal_dim); },   // modules_unc_embed/Embed_0/embedding: [1, G], padded
     k_cfgrl_mods, 1, nullptr, {nullptr, nullptr, nullptr}, cfgrl_leaves,   // (one TrainState: every chunk)
     HI_GLOROT, nullptr, cfgrl_embed_init,
     &fql_engine::build_cfgrl_workspace, [](const fql_engine& e) { return e.bc_macs(); },
     SMP_FLOW, nullptr, {2, false, 0}, nullptr, 0},
};

}  // namespace
const KindDesc& fql_engine::desc() const { return k_kinds[(int)kind]; }

// ================================================================================================
// C ABI
// ================================================================================================
// Which kind of handle may call which entry point: one row per entry point that is not open to every kind, one column per AgentKind.
// A cell is OK_ (admitted), NO_ (refused) or the refusal's hint; an ONLY_ row belongs to that kind alone.  A refusal is
// FQL_E_STATE, "<entry point> is not available on <label> (<hint>)" or "<entry point> needs <label> (<create call>)".
struct Admission {
    const char* name;
    int only;                          // >= 0: that AgentKind alone (the cells are unused)
    const char* refuse[kNumKinds];     // FQL, IFQL, ReBRAC, SAC, BC, IQL, IQL-diffusion, CFGRL
};
#define OK_ nullptr
#define NO_ ""
#define FQL_ALONE {OK_, NO_, NO_, NO_, NO_, NO_, NO_, NO_}
#define ONLY_(k) (int)AgentKind::k, {}
#define EP_TABLE(X) \
    X(update_begin, -1, FQL_ALONE)                                                                                                 \
    X(update_end, -1, FQL_ALONE)                                                                                                   \
    X(update, -1, {OK_, OK_, "its batch has no next_actions: fql_rebrac_update", NO_, NO_, NO_, "the step kind is an argument: fql_iqld_update", "its batch carries actor_goals: fql_cfgrl_update"})                                   \
    X(total_loss, -1, {OK_, OK_, "its batch has no next_actions: fql_rebrac_total_loss", NO_, NO_, NO_, "fql_iqld_total_loss", "fql_cfgrl_policy_loss"})                           \
    X(sample_actions, -1, {OK_, OK_, OK_, OK_, "fql_bc_sample_actions", OK_, "fql_iqld_sample_actions", "it takes goals: fql_cfgrl_sample_actions"})                                                      \
    X(flow_actions, -1, {OK_, OK_, "the actor is deterministic, there is no flow", NO_, NO_, NO_, NO_, NO_})                                 \
    X(module_forward, -1, {OK_, OK_, OK_, OK_, "policy's input carries the host-built time embedding", OK_, OK_, "actor_flow's input carries the goals and the unc_embed row"})  \
    X(noise_from_jax_keys, -1, FQL_ALONE)                                                                                          \
    X(dataset_add_frames, -1, FQL_ALONE)                                                                                           \
    X(replay_create, -1, {OK_, NO_, NO_, OK_, NO_, NO_, NO_, NO_})                                                                           \
    X(replay_add, -1, {OK_, NO_, NO_, OK_, NO_, NO_, NO_, NO_})                                                                              \
    X(replay_add_frames, -1, FQL_ALONE)                                                                                            \
    X(replay_size, -1, {OK_, NO_, NO_, OK_, NO_, NO_, NO_, NO_})                                                                             \
    X(update_balanced, -1, FQL_ALONE)                                                                                              \
    X(update_from_dataset_begin, -1, FQL_ALONE)                                                                                    \
    X(update_from_dataset_begin_split, -1, FQL_ALONE)                                                                              \
    X(update_begin_split, -1, FQL_ALONE)                                                                                           \
    X(update_end_split, -1, FQL_ALONE)                                                                                             \
    X(grad_buckets, -1, FQL_ALONE)                                                                                                 \
    X(update_from_dataset, -1, {OK_, OK_, "the step kind is an argument: fql_rebrac_update_from_dataset", NO_, NO_, NO_, "the step kind is an argument: fql_iqld_update_from_dataset", "the goal draw: fql_cfgrl_update_from_dataset"})          \
    X(info_wait, -1, {OK_, OK_, OK_, "14 infos: fql_info_wait_n", "4 infos: fql_info_wait_n", "16 or 19 infos: fql_info_wait_n", "21 infos: fql_info_wait_n", "4 infos: fql_info_wait_n"})  \
    X(read_info, -1, {OK_, OK_, OK_, "14 infos: fql_read_info_n", "4 infos: fql_read_info_n", "16 or 19 infos: fql_read_info_n", "21 infos: fql_read_info_n", "4 infos: fql_read_info_n"})  \
    X(profile_update, -1, {OK_, OK_, "FQL batch sources only", NO_, NO_, NO_, NO_, NO_})                                                     \
    X(debug_workspace, -1, {OK_, OK_, "FQL workspaces only", NO_, NO_, NO_, NO_, NO_})                                                       \
    X(dataset_upload_frames, -1, FQL_ALONE)                                                                                        \
    X(update_from_frames, -1, FQL_ALONE)                                                                                           \
    X(set_step, -1, {OK_, OK_, OK_, OK_, OK_, OK_, "one count per TrainState: fql_iqld_set_steps", OK_})                                \
    X(set_grad_scale, -1, {OK_, OK_, OK_, OK_, OK_, OK_, "no data-parallel halves on this kind", OK_})                                  \
    X(rebrac_update, ONLY_(REBRAC))                                                                                                \
    X(rebrac_update_from_dataset, ONLY_(REBRAC))                                                                                   \
    X(rebrac_total_loss, ONLY_(REBRAC))                                                                                            \
    X(rebrac_sample_actions, ONLY_(REBRAC))                                                                                        \
    X(rebrac_stats, ONLY_(REBRAC))                                                                                                 \
    X(sac_update, ONLY_(SAC))                                                                                                      \
    X(sac_update_from_dataset, ONLY_(SAC))                                                                                         \
    X(sac_update_balanced, ONLY_(SAC))                                                                                             \
    X(sac_total_loss, ONLY_(SAC))                                                                                                  \
    X(sac_sample_actions, ONLY_(SAC))                                                                                              \
    X(sac_stats, ONLY_(SAC))                                                                                                       \
    X(iql_update, ONLY_(IQL))                                                                                                      \
    X(iql_update_from_dataset, ONLY_(IQL))                                                                                         \
    X(iql_total_loss, ONLY_(IQL))                                                                                                  \
    X(iql_sample_actions, ONLY_(IQL))                                                                                              \
    X(iql_stats, ONLY_(IQL))                                                                                                       \
    X(bc_update, ONLY_(BC))                                                                                                        \
    X(bc_update_from_dataset, ONLY_(BC))                                                                                           \
    X(bc_policy_loss, ONLY_(BC))                                                                                                   \
    X(bc_sample_actions, ONLY_(BC))                                                                                                \
    X(bc_stats, ONLY_(BC))                                                                                                         \
    X(iqld_update, ONLY_(IQLD))                                                                                                    \
    X(iqld_update_from_dataset, ONLY_(IQLD))                                                                                       \
    X(iqld_total_loss, ONLY_(IQLD))                                                                                                \
    X(iqld_sample_actions, ONLY_(IQLD))                                                                                            \
    X(iqld_read_rows, ONLY_(IQLD))                                                                                                 \
    X(iqld_get_steps, ONLY_(IQLD))                                                                                                 \
    X(iqld_set_steps, ONLY_(IQLD))                                                                                                 \
    X(iqld_stats, ONLY_(IQLD))                                                                                                     \
    X(iqld_sample_actions_cfgs, ONLY_(IQLD))                                                                                       \
    X(cfgrl_update, ONLY_(CFGRL))                                                                                                  \
    X(cfgrl_update_from_dataset, ONLY_(CFGRL))                                                                                     \
    X(cfgrl_policy_loss, ONLY_(CFGRL))                                                                                             \
    X(cfgrl_dataset_goals, ONLY_(CFGRL))                                                                                           \
    X(cfgrl_sample_actions, ONLY_(CFGRL))                                                                                          \
    X(cfgrl_read_rows, ONLY_(CFGRL))                                                                                               \
    X(cfgrl_stats, ONLY_(CFGRL))                                                                                                   \
    X(cfgrl_sample_actions_cfgs, ONLY_(CFGRL))                                                                                     \
    X(sample_cfgs_stats, -1, {NO_, NO_, NO_, NO_, NO_, NO_, OK_, OK_})
#define X(ep, ...) EP_##ep,
enum EntryPoint { EP_TABLE(X) EP_COUNT };
#undef X
#define X(ep, ...) {"fql_" #ep, __VA_ARGS__},
static const Admission k_admission[EP_COUNT] = {EP_TABLE(X)};
#undef X
#undef OK_
#undef NO_
#undef FQL_ALONE
#undef ONLY_
// false: h->err says why `h` may not call `ep`
static bool admitted(fql_handle h, EntryPoint ep) {
    const Admission& a = k_admission[ep];
    const KindDesc& d = h->desc();
    if (a.only >= 0) {
        if ((int)h->kind == a.only) return true;
        const KindDesc& o = k_kinds[a.only];
        h->err = std::string(a.name) + " needs " + o.label + " (" + o.create + ")";
        return false;
    }
    const char* hint = a.refuse[(int)h->kind];
    if (!hint) return true;
    h->err = std::string(a.name) + " is not available on " + d.label + (*hint ? std::string(" (") + hint + ")" : std::string());
    return false;
}
// the first line of such an entry point; a null handle passes (the entry point's own check answers it)
#define FQL_ADMIT(h, ep) \
    do { if ((h) && !admitted((h), (ep))) return FQL_E_STATE; } while (0)
// FQL_TRY: every entry point that may use HIP on the engine's buffers - updates still on the engine's AQL queues finish first.
// FQL_TRY_FAST: the update entry points that can go to those queues themselves (run_update decides).
#define FQL_TRY(h, ...) FQL_TRY_(h, ((h)->group_fence(), (h)->hip_touch()), __VA_ARGS__)
#define FQL_TRY_FAST(h, ...) FQL_TRY_(h, (h)->group_fence(), __VA_ARGS__)
#define FQL_TRY_(h, pre, ...)                              \
    try {                                                  \
        pre;                                               \
        __VA_ARGS__;                                       \
        return FQL_OK;                                     \
    } catch (const Invalid& e) {                           \
        (h)->err = e.msg;                                  \
        return FQL_E_INVALID;                              \
    } catch (const HipError& e) {                          \
        (h)->err = e.msg;                                  \
        return FQL_E_HIP;                                  \
    } catch (const std::exception& e) {                    \
        (h)->err = e.what();                               \
        return FQL_E_HIP;                                  \
    }

// ---- online fine-tuning: ring capacity, uint8 ring insert, the replay ring of balanced sampling ---------------------------------
namespace {
// copy `rows` rows of `w` elements into a fresh zero-filled allocation of `cap` rows; frees the old one
template <typename T>
void regrow(T*& p, int64_t rows, int64_t cap, size_t w) {
    T* q = nullptr;
    HIP_CHECK(hipMalloc((void**)&q, (size_t)cap * w * sizeof(T)));
    HIP_CHECK(hipMemset(q, 0, (size_t)cap * w * sizeof(T)));
    if (p && rows > 0) HIP_CHECK(hipMemcpy(q, p, (size_t)rows * w * sizeof(T), hipMemcpyDeviceToDevice));
    if (p) hipFree(p);
    p = q;
}
}  // namespace

// one transition into row `pos` of a ring: the float fields through the staging row + fql_dataset_add_kernel, frames as two byte copies
static void ring_insert(fql_handle h, float* obs, float* act, float* rew, float* mask, float* nobs, unsigned char* frames,
                        unsigned char* next_frames, int64_t pos, const float* ob, const float* ac, float reward, float m,
                        const float* nob, const uint8_t* frame, const uint8_t* next_frame) {
    const int od = frames ? 0 : h->cfg.obs_dim, ad = h->cfg.act_dim;   // frames rings keep no float observations
    if (od > 1024) invalid("obs_dim too large for the ring-insert kernel");
    if (!h->ds_row) HIP_CHECK(hipMalloc((void**)&h->ds_row, (size_t)(2 * h->cfg.obs_dim + ad + 2) * sizeof(float)));
    std::vector<float> row(2 * od + ad + 2);
    if (od) std::memcpy(row.data(), ob, od * sizeof(float));
    std::memcpy(row.data() + od, ac, ad * sizeof(float));
    row[od + ad] = reward; row[od + ad + 1] = m;
    if (od) std::memcpy(row.data() + od + ad + 2, nob, od * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(h->ds_row, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(fql_dataset_add_kernel, dim3(1), dim3(std::max(64, pad16(std::max(od, ad)))), 0, h->stream, obs, act, rew, mask, nobs,
                       h->ds_row, pos, od, ad);
    HIP_CHECK(hipGetLastError());
    if (frames) {
        const size_t fb = (size_t)h->cfg.img_h * h->cfg.img_w * (h->cfg.img_c / h->ds_fs);
        HIP_CHECK(hipMemcpyAsync(frames + (size_t)pos * fb, frame, fb, hipMemcpyDefault, h->stream));
        HIP_CHECK(hipMemcpyAsync(next_frames + (size_t)pos * fb, next_frame, fb, hipMemcpyDefault, h->stream));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));   // the caller's buffers are borrowed for the call only
}

extern "C" {

const char* fql_info_name(int i) { return (i >= 0 && i < FQL_NUM_INFO) ? k_info_names[i] : ""; }
int fql_abi_version(void) { return FQL_ABI_VERSION; }

void fql_default_config(fql_config* c) {
    std::memset(c, 0, sizeof *c);
    c->num_actor_hidden = 4; c->num_value_hidden = 4;
    for (int i = 0; i < 4; ++i) c->actor_hidden[i] = c->value_hidden[i] = 512;
    c->layer_norm = 1; c->actor_layer_norm = 0;
    c->lr = 3e-4f; c->discount = 0.99f; c->tau = 0.005f; c->alpha = 300.0f;
    c->q_agg = 0; c->flow_steps = 10; c->normalize_q_loss = 0; c->batch_size = 256; c->precision = 0;
}

const char* fql_last_error(fql_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

struct AgentSpec {
    AgentKind kind;
    const void* cfg;   // that kind's config struct (fql_ifql_config, ...); FQL has none
};
static int create_engine(const fql_config* cfg, AgentSpec agent, uint64_t seed, fql_handle* out);
int fql_create(const fql_config* cfg, uint64_t seed, fql_handle* out) { return create_engine(cfg, {AgentKind::FQL, nullptr}, seed, out); }

void fql_ifql_default_config(fql_ifql_config* c) {   // agents/ifql.py:231-250
    std::memset(c, 0, sizeof *c);
    c->expectile = 0.9f;
    c->num_samples = 32;
}
int fql_ifql_create(const fql_config* cfg, const fql_ifql_config* icfg, uint64_t seed, fql_handle* out) {
    if (!icfg) { g_create_error = "icfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::IFQL, icfg}, seed, out);
}
void fql_rebrac_default_config(fql_rebrac_config* c) {   // agents/rebrac.py:222-244
    std::memset(c, 0, sizeof *c);
    c->alpha_actor = 0.0f;
    c->alpha_critic = 0.0f;
    c->actor_noise = 0.2f;
    c->actor_noise_clip = 0.5f;
    c->tanh_squash = 1;
    c->actor_fc_scale = 0.01f;
}
int fql_rebrac_create(const fql_config* cfg, const fql_rebrac_config* rcfg, uint64_t seed, fql_handle* out) {
    if (!rcfg) { g_create_error = "rcfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::REBRAC, rcfg}, seed, out);
}
void fql_sac_default_config(fql_sac_config* c) {   // agents/sac.py get_config
    std::memset(c, 0, sizeof *c);
    c->target_entropy = NAN;
    c->target_entropy_multiplier = 0.5f;
    c->tanh_squash = 1;
    c->state_dependent_std = 1;
    c->actor_fc_scale = 0.01f;
    c->backup_entropy = 0;
}
int fql_sac_create(const fql_config* cfg, const fql_sac_config* scfg, uint64_t seed, fql_handle* out) {
    if (!scfg) { g_create_error = "scfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::SAC, scfg}, seed, out);
}
int fql_num_info(fql_handle h) { return h ? h->num_info() : FQL_E_INVALID; }
const char* fql_handle_info_name(fql_handle h, int i) { return (!h || i < 0 || i >= h->num_info()) ? nullptr : h->info_names()[i]; }

static int create_engine(const fql_config* cfg, AgentSpec agent, uint64_t seed, fql_handle* out) {
    if (!cfg || !out) { g_create_error = "cfg/out must not be NULL"; return FQL_E_INVALID; }
    *out = nullptr;
    const AgentKind kind = agent.kind;
    const KindDesc& kd = k_kinds[(int)kind];
    auto refuse = [&](const std::string& why) { g_create_error = std::string(kd.create) + ": " + why; return FQL_E_INVALID; };
    if (!(kd.traits & K_VISUAL)) {   // state observations and fp32 only
        if (cfg->encoder != 0) return refuse(std::string("visual encoders are not available for ") + kd.name + " (encoder must be 0)");
        if (cfg->precision != 0) return refuse(std::string(kd.name) + " runs in fp32 only (precision must be 0)");
    }
    if (const char* why = kd.check ? kd.check(agent.cfg) : nullptr) return refuse(why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        g_create_error = "no HIP device visible: the FQL engine has no CPU fallback";
        return FQL_E_NODEVICE;
    }
    auto* h = new fql_engine();
    try {
        h->cfg = *cfg;
        h->seed = seed;
        h->kind = kind;
        if (kd.adopt) kd.adopt(*h, agent.cfg);
        if (cfg->encoder != 0) {   // visual agent (agents/fql.py:196-202): the MLPs see the 512-wide encoding instead of obs
            if (cfg->encoder != 1 && cfg->encoder != 2) invalid("encoder %d not available (0 = none, 1 = impala_small, 2 = impala)", cfg->encoder);
            if (cfg->img_h <= 0 || cfg->img_w <= 0 || cfg->img_h % 32 || cfg->img_w % 32 || cfg->img_w > 128 || cfg->img_c <= 0 || cfg->img_c > 16)
                invalid("image shape must be [H, W, C] with H, W multiples of 32 (W <= 128) and C <= 16 (got %d, %d, %d)", cfg->img_h,
                        cfg->img_w, cfg->img_c);
            {   // the uint8 first layer stages (R + 2) image rows as <= 4 dwords per thread (ConvTile::NU8)
                const int R0 = std::min(cfg->img_h, std::max(1, 128 / cfg->img_w));
                if ((R0 + 2) * cfg->img_w * cfg->img_c > 4096 || (cfg->img_w * cfg->img_c) % 4)
                    invalid("image rows of %d x %d channels are too wide for the first-layer kernel", cfg->img_w, cfg->img_c);
            }
            h->visual = true;
            h->enc_dim = 512;          // mlp_hidden_dims = (512,) (utils/encoders.py:69)
            h->cfg.obs_dim = h->enc_dim;
            cfg = &h->cfg;
        }
        if (cfg->obs_dim <= 0 || cfg->act_dim <= 0) invalid("obs_dim and act_dim must be positive (got %d, %d)", cfg->obs_dim, cfg->act_dim);
        if (cfg->num_actor_hidden < 1 || cfg->num_actor_hidden > FQL_MAX_HIDDEN || cfg->num_value_hidden < 1 || cfg->num_value_hidden > FQL_MAX_HIDDEN)
            invalid("hidden layer counts must be in [1, %d]", FQL_MAX_HIDDEN);
        if (cfg->flow_steps < 1) invalid("flow_steps must be >= 1");
        if (cfg->q_agg != 0 && cfg->q_agg != 1) invalid("q_agg must be 0 (mean) or 1 (min)");
        if (cfg->precision != 0 && cfg->precision != 2) invalid("precision %d not available (0 = fp32 MFMA, 2 = bf16 x 3 split MFMA)", cfg->precision);
        HIP_CHECK(hipGetDevice(&h->device));
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, h->device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            g_create_error = std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 (MI355X) only";
            delete h;
            return FQL_E_NODEVICE;
        }
        // (stream priorities were tried for the graph lanes in round 1: no gain with two streams, a 4x slowdown with three)
        h->num_cus = prop.multiProcessorCount;
        // (stream priorities and CU masks were tried for the graph lanes in rounds 1-2: no gain with two streams, a 4x slowdown with three)
        HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        for (int l = 1; l < FQL_LANES; ++l) HIP_CHECK(hipStreamCreateWithFlags(&h->lane_streams[l], hipStreamNonBlocking));
        h->build_nets();
        if (h->has(K_TIME_TABLE)) {   // the timestep-embedding table, rows k = 0..S: freq_i = float32(exp_f64(-ln(10000) i / 8)),
                       // arg = float32(float32(t 10000) freq_i), [cos | sin] in fp64 of that fp32 argument, rounded to fp32
            const int S = h->bc_steps;
            std::vector<float> tab((size_t)(S + 1) * BC_EMB);
            for (int k = 0; k <= S; ++k) {
                const float t = (float)k / (float)S;
                const float ts = t * 10000.0f;
                for (int i = 0; i < BC_EMB / 2; ++i) {
                    const float freq = (float)std::exp(-std::log(10000.0) * (double)i / (double)(BC_EMB / 2));
                    const float arg = ts * freq;
                    tab[(size_t)k * BC_EMB + i] = (float)std::cos((double)arg);
                    tab[(size_t)k * BC_EMB + BC_EMB / 2 + i] = (float)std::sin((double)arg);
                }
            }
            HIP_CHECK(hipMalloc((void**)&h->d_emb, tab.size() * sizeof(float)));
            HIP_CHECK(hipMemcpy(h->d_emb, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        HIP_CHECK(hipMalloc((void**)&h->P, h->n_total * sizeof(float)));
        HIP_CHECK(hipMalloc((void**)&h->G, h->n_train * sizeof(float)));
        HIP_CHECK(hipMalloc((void**)&h->Mu, h->n_train * sizeof(float)));
        HIP_CHECK(hipMalloc((void**)&h->Nu, h->n_train * sizeof(float)));
        HIP_CHECK(hipMemset(h->G, 0, h->n_train * sizeof(float)));
        HIP_CHECK(hipMemset(h->Mu, 0, h->n_train * sizeof(float)));
        HIP_CHECK(hipMemset(h->Nu, 0, h->n_train * sizeof(float)));
        h->build_enc_weights();
        h->build_leaves();
        h->init_params();
        h->build_chain_weights();
        h->refresh_chain_weights(h->stream);
        HIP_CHECK(hipMalloc((void**)&h->d_state, sizeof(DevState)));
        if (h->own_info()) {
            HIP_CHECK(hipMalloc((void**)&h->iql_info, 2 * IQL_INFO_STRIDE * sizeof(float)));
            HIP_CHECK(hipMemset(h->iql_info, 0, 2 * IQL_INFO_STRIDE * sizeof(float)));
        }
        HIP_CHECK(hipMalloc((void**)&h->d_src, sizeof(SrcDesc)));
        HIP_CHECK(hipHostMalloc((void**)&h->h_src_ring, 64 * sizeof(SrcDesc), hipHostMallocDefault));
        HIP_CHECK(hipHostMalloc((void**)&h->h_info_ring, fql_engine::kInfoRing * 32 * sizeof(float), hipHostMallocDefault));
        for (auto& e : h->info_ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        DevState st{};
        st.rng_step = 0; st.adam_count = 0; st.train_step = 1; st.b1pow = 1.0; st.b2pow = 1.0; st.grad_scale = 1.0f; st.lam = 1.0f;
        const float ninf = -INFINITY, pinf = INFINITY;
        int bi; std::memcpy(&bi, &ninf, 4); st.gmax = bi >= 0 ? bi : bi ^ 0x7FFFFFFF;
        std::memcpy(&bi, &pinf, 4); st.gmin = bi >= 0 ? bi : bi ^ 0x7FFFFFFF;
        HIP_CHECK(hipMemcpy(h->d_state, &st, sizeof st, hipMemcpyHostToDevice));
        if (h->has(K_ACTOR_STATE)) {   // the actor TrainState's counters (the same initial values)
            HIP_CHECK(hipMalloc((void**)&h->d_state_a, sizeof(DevState)));
            HIP_CHECK(hipMemcpy(h->d_state_a, &st, sizeof st, hipMemcpyHostToDevice));
        }
        if (h->has(K_GOALS)) {
            HIP_CHECK(hipMalloc((void**)&h->d_gsrc, sizeof(CfgrlSrc)));
            HIP_CHECK(hipMemset(h->d_gsrc, 0, sizeof(CfgrlSrc)));
            HIP_CHECK(hipHostMalloc((void**)&h->h_gsrc_ring, 64 * sizeof(CfgrlSrc), hipHostMallocDefault));
        }
        h->build_workspace(cfg->batch_size);
    } catch (const Invalid& e) {
        g_create_error = e.msg; fql_destroy(h); return FQL_E_INVALID;
    } catch (const HipError& e) {
        g_create_error = e.msg; fql_destroy(h); return FQL_E_HIP;
    }
    *out = h;
    return FQL_OK;
}

int fql_destroy(fql_handle h) {
    if (!h) return FQL_OK;
    if (h->group) { h->err = "fql_destroy: the handle is a member of an agent group (fql_group_destroy first)"; return FQL_E_STATE; }
    try { h->aql_drain(); } catch (...) {}
    if (h->stream) hipStreamSynchronize(h->stream);
    hipDeviceSynchronize();
    h->free_workspace();
    h->aql.shutdown();
    for (auto& kv : h->evals)
        for (void* p : kv.second->allocs) hipFree(p);
    for (auto& kv : h->queries)
        for (void* p : kv.second->allocs) hipFree(p);
    hipFree(h->P); hipFree(h->G); hipFree(h->Mu); hipFree(h->Nu); hipFree(h->d_chunks); hipFree(h->d_partials); hipFree(h->d_ticket); hipFree(h->d_leaf_range); hipFree(h->d_state); hipFree(h->d_src); hipFree(h->d_emb); hipFree(h->iql_info); hipFree(h->d_state_a);
    if (h->h_src_ring) hipHostFree(h->h_src_ring);
    hipFree(h->d_gsrc); hipFree(h->ds_final); hipFree(h->ds_reps);
    if (h->h_gsrc_ring) hipHostFree(h->h_gsrc_ring);
    if (h->h_info_ring) hipHostFree(h->h_info_ring);
    for (auto& e : h->info_ev) if (e) hipEventDestroy(e);
    hipFree(h->ds_obs); hipFree(h->ds_act); hipFree(h->ds_rew); hipFree(h->ds_mask); hipFree(h->ds_nobs); hipFree(h->ds_row);
    hipFree(h->ds_frames); hipFree(h->ds_next_frames); hipFree(h->ds_init);
    hipFree(h->rb_obs); hipFree(h->rb_act); hipFree(h->rb_rew); hipFree(h->rb_mask); hipFree(h->rb_nobs);
    hipFree(h->rb_frames); hipFree(h->rb_next_frames); hipFree(h->rb_init);
    for (void* q : h->enc_allocs) hipFree(q);
    for (void* q : h->chain_allocs) hipFree(q);
    if (h->stream) hipStreamDestroy(h->stream);
    for (hipStream_t s : h->lane_streams) if (s) hipStreamDestroy(s);
    delete h;
    return FQL_OK;
}

int fql_set_batch_size(fql_handle h, int batch_size) {
    if (!h) return FQL_E_INVALID;
    if (h->group) { h->err = "fql_set_batch_size: the handle is a member of an agent group (fql_group_destroy first)"; return FQL_E_STATE; }
    FQL_TRY(h, { if (batch_size != h->B) h->build_workspace(batch_size); });
}

int fql_num_leaves(fql_handle h) { return h ? (int)h->leaves.size() : FQL_E_INVALID; }

int fql_leaf_info(fql_handle h, int index, char* name, int name_cap, int* ndim, int64_t shape[4]) {
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (index < 0 || index >= (int)h->leaves.size()) invalid("leaf index %d out of range", index);
        const Leaf& l = h->leaves[index];
        if (name && name_cap > 0) { std::strncpy(name, l.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
        if (ndim) *ndim = l.ndim;
        if (shape) for (int i = 0; i < 4; ++i) shape[i] = l.shape[i];
    });
}

static int leaf_rw(fql_handle h, const char* leaf, float* host, size_t n, int which, bool to_device) {
    if (!h) return FQL_E_INVALID;
    try {
        h->group_fence();
        h->hip_touch();   // stream-less updates still on the AQL queues read and write P / Mu / Nu; a chain-weight refresh must precede the next submit
        if (!leaf || !host) invalid("leaf/host pointer must not be NULL");
        const Leaf* l = h->find_leaf(leaf);
        if (!l) { h->err = std::string("unknown leaf: ") + leaf; return FQL_E_NOTFOUND; }
        if (n != fql_engine::leaf_count(*l)) invalid("leaf %s has %zu elements, got %zu", leaf, fql_engine::leaf_count(*l), n);
        float* arena = h->P;
        if (which >= 0) {
            if (!l->trainable && which >= 0) {
                // optax keeps (zero-gradient) moments for the target leaves too; they stay exactly 0
                if (to_device) return FQL_OK;
                std::memset(host, 0, n * sizeof(float));
                return FQL_OK;
            }
            arena = which == 0 ? h->Mu : h->Nu;
        }
        h->leaf_io(*l, arena, host, to_device);
        if (to_device && which < 0 && l->name.rfind("modules_actor_bc_flow/", 0) == 0) h->refresh_chain_weights(h->stream);
        return FQL_OK;
    } catch (const Invalid& e) { h->err = e.msg; return FQL_E_INVALID; }
    catch (const HipError& e) { h->err = e.msg; return FQL_E_HIP; }
}
int fql_get_param(fql_handle h, const char* leaf, float* out, size_t n) { return leaf_rw(h, leaf, out, n, -1, false); }
int fql_set_param(fql_handle h, const char* leaf, const float* in, size_t n) { return leaf_rw(h, leaf, const_cast<float*>(in), n, -1, true); }
int fql_get_opt_state(fql_handle h, int which, const char* leaf, float* out, size_t n) {
    if (which != 0 && which != 1) return FQL_E_INVALID;
    return leaf_rw(h, leaf, out, n, which, false);
}
int fql_set_opt_state(fql_handle h, int which, const char* leaf, const float* in, size_t n) {
    if (which != 0 && which != 1) return FQL_E_INVALID;
    return leaf_rw(h, leaf, const_cast<float*>(in), n, which, true);
}

int fql_get_step(fql_handle h, int64_t* adam_count, int64_t* train_step) {
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipDeviceSynchronize());
        DevState st;
        HIP_CHECK(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));
        if (adam_count) *adam_count = st.adam_count;
        if (train_step) *train_step = st.train_step;
    });
}
int fql_set_step(fql_handle h, int64_t adam_count, int64_t train_step) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_set_step);   // (an IQL-diffusion handle keeps a second counter block, which this call does not write)
    FQL_TRY(h, {
        if (adam_count < 0) invalid("adam_count must be >= 0");
        HIP_CHECK(hipDeviceSynchronize());
        DevState st;
        HIP_CHECK(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));
        st.adam_count = adam_count; st.train_step = train_step;
        st.rng_step = (uint64_t)adam_count;   // every update advances both: a restored agent draws what the saved one would have drawn next
        st.b1pow = std::pow(0.9, (double)adam_count); st.b2pow = std::pow(0.999, (double)adam_count);
        HIP_CHECK(hipMemcpy(h->d_state, &st, sizeof st, hipMemcpyHostToDevice));
    });
}

// NULL = the engine's own stream; FQL_STREAM_LEGACY ((void*)1 == hipStreamLegacy) = the legacy default stream, i.e. the stream
// torch's *default* stream maps to (its handle reads 0, which cannot be told from "no stream" here); anything else is a hipStream_t.
static hipStream_t pick(fql_handle h, void* s) { return s ? (hipStream_t)s : h->stream; }

// FQL_NO_GRAPH (diagnostics; the captured graph is the product path): 1 = eager launches on one stream, 2 = eager launches on the lane
// streams (tests/test_gpu_streams.py runs the parity suite under it); any other non-zero value acts as 1
static int no_graph() {
    static const int v = getenv("FQL_NO_GRAPH") ? atoi(getenv("FQL_NO_GRAPH")) : 0;
    return v;
}

static void run_program(fql_handle h, Program& pr, hipStream_t s) {
    if (no_graph() == 2) h->run_launches(pr, s, h->lane_streams);
    else if (no_graph()) h->run_launches(pr, s);
    else HIP_CHECK(hipGraphLaunch(pr.exec, s));
}

// One update: `pr` is prog_full (FQL, IFQL, a full ReBRAC step) or prog_critic (a critic-only ReBRAC step).  The caller left the stream to
// the engine: the program's AQL form on the engine's own queues (fql_aql.h; built by the first such update, the stream drained first if
// HIP work may be pending on it).  Otherwise, or when that path is off: the captured graph on `s`.
static void run_update(fql_handle h, Program& pr, hipStream_t s, bool own_stream) {
    require_graph(pr);
    if (own_stream && !no_graph()) {
        if (!pr.aql_tried) {
            pr.aql_tried = true;
            h->hip_touch();
            h->build_aql(pr);
        }
        if (pr.aql.ok) {
            if (h->hip_dirty) { HIP_CHECK(hipStreamSynchronize(s)); h->hip_dirty = false; }
            try { h->aql.submit(pr.aql); } catch (const AqlError& e) { throw HipError{e.msg}; }
            h->last_update_aql = true;
            return;
        }
    }
    h->last_update_aql = false;
    h->hip_touch();
    run_program(h, pr, s);
}
// The body of every entry point that is one whole update: source(s) points the step at its batch, `pr` runs through run_update, and
// the first n_info infos go to `info` (null: none).
extern "C++" {
template <typename Source>
static int update_with(fql_handle h, Program& pr, float* info, int n_info, void* stream, Source&& source) {
    FQL_TRY_FAST(h, {
        hipStream_t s = pick(h, stream);
        source(s);
        run_update(h, pr, s, stream == nullptr);
        h->finish_info(info, n_info, s);
    });
}
}

int fql_update_begin(fql_handle h, const float* obs, const float* act, const float* rew, const float* mask,
                     const float* nobs, int batch_size, const fql_noise* noise, void* stream) {
    FQL_ADMIT(h, EP_update_begin);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->source_from_batch(obs, act, rew, mask, nobs, batch_size, noise, 1, s);
        run_program(h, h->prog_fwdbwd, s);
        h->began = true;
        h->split_begun = false;
    });
}
int fql_update_end(fql_handle h, float* info13, void* stream) {
    FQL_ADMIT(h, EP_update_end);
    if (!h) return FQL_E_INVALID;
    if (!h->began) { h->err = "fql_update_end without fql_update_begin"; return FQL_E_STATE; }
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        run_program(h, h->prog_opt, s);
        h->began = false;
        h->finish_info(info13, FQL_NUM_INFO, s);
    });
}
int fql_update(fql_handle h, const float* obs, const float* act, const float* rew, const float* mask, const float* nobs,
               int batch_size, const fql_noise* noise, float* info13, void* stream) {
    FQL_ADMIT(h, EP_update);
    if (h && !h->began) {
        return update_with(h, h->prog_full, info13, FQL_NUM_INFO, stream, [&](hipStream_t s) {
            h->source_from_batch(obs, act, rew, mask, nobs, batch_size, noise, 1, s);
        });
    }
    int rc = fql_update_begin(h, obs, act, rew, mask, nobs, batch_size, noise, stream);
    if (rc != FQL_OK) return rc;
    return fql_update_end(h, info13, stream);
}
int fql_grad_buffer(fql_handle h, void** device_ptr, size_t* num_floats) {
    if (!h || !device_ptr || !num_floats) return FQL_E_INVALID;
    *device_ptr = h->G;
    *num_floats = h->n_train;
    return FQL_OK;
}
int fql_set_grad_scale(fql_handle h, float scale) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_set_grad_scale);   // (the actor's Adam launch of an IQL-diffusion handle reads the scale of its own counter block)
    FQL_TRY(h, {
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(&h->d_state->grad_scale, &scale, sizeof scale, hipMemcpyHostToDevice));
    });
}

int fql_set_rng_stream(fql_handle h, uint64_t stream_id) {
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(&h->d_state->rng_stream, &stream_id, sizeof stream_id, hipMemcpyHostToDevice));
    });
}

int fql_total_loss(fql_handle h, const float* obs, const float* act, const float* rew, const float* mask, const float* nobs,
                   int batch_size, const fql_noise* noise, float* loss, float* info10, void* stream) {
    FQL_ADMIT(h, EP_total_loss);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->source_from_batch(obs, act, rew, mask, nobs, batch_size, noise, 0, s);
        run_program(h, h->prog_loss, s);
        float tmp[10];
        HIP_CHECK(hipMemcpyAsync(tmp, &h->d_state->info[0], sizeof tmp, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const KindDesc& kd = h->desc();   // (FQL: critic + actor, ten infos; IFQL: value + critic + actor, nine)
        float sum = tmp[kd.probe_terms[0]];
        for (int i = 1; i < 3 && kd.probe_terms[i] >= 0; ++i) sum += tmp[kd.probe_terms[i]];
        if (loss) *loss = sum;
        if (info10) std::memcpy(info10, tmp, (size_t)kd.probe_infos * sizeof(float));
    });
}

int fql_sample_actions(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, float* out, void* stream) {
    FQL_ADMIT(h, EP_sample_actions);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, h->sample(obs, noise, seed, 1.0f, n, out, pick(h, stream), stream == nullptr));
}
int fql_flow_actions(fql_handle h, const float* obs, const float* noises, int n, float* out, void* stream) {
    FQL_ADMIT(h, EP_flow_actions);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, h->eval_rows(true, obs, noises, 0, n, out, pick(h, stream), stream == nullptr));
}
int fql_module_forward(fql_handle h, const char* module, const float* obs, const float* act, const float* times, int n, float* out,
                       void* stream) {
    FQL_ADMIT(h, EP_module_forward);
    if (!h) return FQL_E_INVALID;
    if (h->visual) {
        h->err = "fql_module_forward is not available on a visual agent (the reference runs the module's encoder first: state observations only)";
        return FQL_E_STATE;
    }
    if (!module) { h->err = "fql_module_forward: module must not be NULL"; return FQL_E_INVALID; }
    const auto mods = h->modules();
    int mi = -1;
    for (int i = 0; i < (int)mods.size(); ++i)
        if (!std::strcmp(mods[i].name, module)) mi = i;
    if (mi < 0) {
        h->err = std::string("fql_module_forward: ") + h->desc().label + " has no module '" + module + "' (its modules:";
        for (const auto& m : mods) h->err += std::string(" ") + m.name;
        h->err += ")";
        return FQL_E_NOTFOUND;
    }
    FQL_TRY(h, h->module_forward(mi, mods[mi], obs, act, times, n, out, pick(h, stream), stream == nullptr));
}

int fql_dataset_upload(fql_handle h, int64_t n, int64_t capacity, const float* obs, const float* act, const float* rew,
                       const float* mask, const float* nobs) {
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (n < 0 || capacity < std::max<int64_t>(n, 1)) invalid("need capacity >= max(n, 1) (n=%lld capacity=%lld)", (long long)n, (long long)capacity);
        if (n > 0 && (!obs || !act || !rew || !mask || !nobs)) invalid("dataset pointers must not be NULL");
        HIP_CHECK(hipDeviceSynchronize());
        hipFree(h->ds_obs); hipFree(h->ds_act); hipFree(h->ds_rew); hipFree(h->ds_mask); hipFree(h->ds_nobs);
        h->ds_obs = h->ds_act = h->ds_rew = h->ds_mask = h->ds_nobs = nullptr;
        const int od = h->cfg.obs_dim, ad = h->cfg.act_dim;
        auto up = [&](float*& dst, const float* src, size_t w) {
            HIP_CHECK(hipMalloc((void**)&dst, (size_t)capacity * w * sizeof(float)));
            HIP_CHECK(hipMemset(dst, 0, (size_t)capacity * w * sizeof(float)));
            if (n > 0) HIP_CHECK(hipMemcpy(dst, src, (size_t)n * w * sizeof(float), hipMemcpyDefault));
        };
        up(h->ds_obs, obs, od); up(h->ds_act, act, ad); up(h->ds_rew, rew, 1); up(h->ds_mask, mask, 1); up(h->ds_nobs, nobs, od);
        if (!h->ds_row) HIP_CHECK(hipMalloc((void**)&h->ds_row, (size_t)(2 * od + ad + 2) * sizeof(float)));
        h->ds_size = n; h->ds_cap = capacity; h->ds_ptr = n % capacity;
        h->src_valid = false;
        h->drop_goal_table();   // (a CFGRL handle's table describes the rows it was built for)
    });
}
int fql_dataset_add(fql_handle h, const float* ob, const float* ac, float reward, float mask, const float* nob) {
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (!h->ds_obs) throw Invalid{"no dataset allocated (fql_dataset_upload)"};
        if (!ob || !ac || !nob) invalid("transition pointers must not be NULL");
        const int od = h->cfg.obs_dim, ad = h->cfg.act_dim;
        if (od > 1024) invalid("obs_dim too large for the ring-insert kernel");
        std::vector<float> row(2 * od + ad + 2);
        std::memcpy(row.data(), ob, od * sizeof(float));
        std::memcpy(row.data() + od, ac, ad * sizeof(float));
        row[od + ad] = reward; row[od + ad + 1] = mask;
        std::memcpy(row.data() + od + ad + 2, nob, od * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(h->ds_row, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(fql_dataset_add_kernel, dim3(1), dim3(std::max(64, pad16(std::max(od, ad)))), 0, h->stream, h->ds_obs,
                           h->ds_act, h->ds_rew, h->ds_mask, h->ds_nobs, h->ds_row, h->ds_ptr, od, ad);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->drop_goal_table();
        // utils/datasets.py:489-491
        h->ds_ptr = (h->ds_ptr + 1) % h->ds_cap;
        h->ds_size = std::max(h->ds_ptr, h->ds_size);
    });
}
int fql_dataset_size(fql_handle h, int64_t* size, int64_t* pointer) {
    if (!h) return FQL_E_INVALID;
    if (size) *size = h->ds_size;
    if (pointer) *pointer = h->ds_ptr;
    return FQL_OK;
}
// ---- online fine-tuning: ring capacity, uint8 ring insert, the replay ring of balanced sampling (helpers above extern "C")
int fql_noise_from_jax_keys(fql_handle h, const uint32_t* keys10, int partitionable, int batch_size, fql_noise* out, void* stream) {
    FQL_ADMIT(h, EP_noise_from_jax_keys);
    if (!h || !keys10 || !out) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (batch_size != h->B) invalid("batch_size %d does not match the engine's workspace (%d); call fql_set_batch_size", batch_size, h->B);
        hipStream_t s = pick(h, stream);
        const int B = h->B, ad = h->cfg.act_dim;
        JaxNoiseArgs a{};
        for (int w = 0; w < 5; ++w) {
            a.key[w][0] = keys10[2 * w]; a.key[w][1] = keys10[2 * w + 1];
            a.out[w] = h->in_noise[w];
            a.n[w] = w == 2 ? B : B * ad;
        }
        a.partitionable = partitionable ? 1 : 0;
        hipLaunchKernelGGL(fql_jax_noise_kernel, dim3((B * ad + FQL_THREADS - 1) / FQL_THREADS, 5), dim3(FQL_THREADS), 0, s, a);
        HIP_CHECK(hipGetLastError());
        out->eps1 = h->in_noise[0]; out->x0 = h->in_noise[1]; out->t = h->in_noise[2]; out->z = h->in_noise[3]; out->eps2 = h->in_noise[4];
    });
}
int fql_dataset_reserve(fql_handle h, int64_t capacity) {
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        const bool fr = h->visual;
        if (!(fr ? (void*)h->ds_frames : (void*)h->ds_obs)) throw Invalid{"fql_dataset_reserve: no dataset uploaded"};
        if (capacity < h->ds_cap) invalid("fql_dataset_reserve: capacity %lld below the current %lld rows", (long long)capacity, (long long)h->ds_cap);
        if (capacity == h->ds_cap) return FQL_OK;
        HIP_CHECK(hipDeviceSynchronize());
        const int od = h->cfg.obs_dim, ad = h->cfg.act_dim;
        const int64_t rows = h->ds_cap;
        regrow(h->ds_act, rows, capacity, ad); regrow(h->ds_rew, rows, capacity, 1); regrow(h->ds_mask, rows, capacity, 1);
        if (fr) {
            const size_t fb = (size_t)h->cfg.img_h * h->cfg.img_w * (h->cfg.img_c / h->ds_fs);
            regrow(h->ds_frames, rows, capacity, fb); regrow(h->ds_next_frames, rows, capacity, fb);
            // Dataset.__init__ computes initial_locs once (utils/datasets.py:58-62); rows inserted later fall behind the LAST initial
            // location of the initial data (searchsorted(..., side='right') - 1, utils/datasets.py:75) - kept as the reference has it
            std::vector<int64_t> init((size_t)capacity);
            HIP_CHECK(hipMemcpy(init.data(), h->ds_init, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost));
            int64_t last = 0;
            for (int64_t i = 0; i < rows; ++i) last = std::max(last, init[i]);
            for (int64_t i = rows; i < capacity; ++i) init[i] = last;
            hipFree(h->ds_init); h->ds_init = nullptr;
            HIP_CHECK(hipMalloc((void**)&h->ds_init, (size_t)capacity * sizeof(int64_t)));
            HIP_CHECK(hipMemcpy(h->ds_init, init.data(), (size_t)capacity * sizeof(int64_t), hipMemcpyHostToDevice));
        } else {
            regrow(h->ds_obs, rows, capacity, od); regrow(h->ds_nobs, rows, capacity, od);
        }
        h->ds_cap = capacity;
        h->ds_ptr = h->ds_size % capacity;
        h->src_valid = false;
    });
}
int fql_dataset_add_frames(fql_handle h, const uint8_t* frame, const uint8_t* next_frame, const float* ac, float reward, float mask) {
    FQL_ADMIT(h, EP_dataset_add_frames);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (!h->visual || !h->ds_frames) throw Invalid{"no frames dataset allocated (fql_dataset_upload_frames)"};
        if (!frame || !next_frame || !ac) invalid("transition pointers must not be NULL");
        ring_insert(h, nullptr, h->ds_act, h->ds_rew, h->ds_mask, nullptr, h->ds_frames, h->ds_next_frames, h->ds_ptr, nullptr, ac, reward, mask,
                    nullptr, frame, next_frame);
        h->ds_ptr = (h->ds_ptr + 1) % h->ds_cap;          // utils/datasets.py:489-491
        h->ds_size = std::max(h->ds_ptr, h->ds_size);
    });
}
int fql_replay_create(fql_handle h, int64_t capacity) {
    FQL_ADMIT(h, EP_replay_create);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (capacity < 1) invalid("fql_replay_create: capacity %lld", (long long)capacity);
        if (h->visual && !h->ds_frames) throw Invalid{"fql_replay_create: upload the frames dataset first (frame_stack and p_aug are shared, main.py:117-120)"};
        HIP_CHECK(hipDeviceSynchronize());
        const int od = h->cfg.obs_dim, ad = h->cfg.act_dim;
        regrow(h->rb_act, 0, capacity, ad); regrow(h->rb_rew, 0, capacity, 1); regrow(h->rb_mask, 0, capacity, 1);
        if (h->visual) {
            const size_t fb = (size_t)h->cfg.img_h * h->cfg.img_w * (h->cfg.img_c / h->ds_fs);
            regrow(h->rb_frames, 0, capacity, fb); regrow(h->rb_next_frames, 0, capacity, fb);
            regrow(h->rb_init, 0, capacity, 1);   // ReplayBuffer.create: terminals all zero => initial_locs = [0] (utils/datasets.py:58-62)
        } else {
            regrow(h->rb_obs, 0, capacity, od); regrow(h->rb_nobs, 0, capacity, od);
        }
        h->rb_cap = capacity; h->rb_size = 0; h->rb_ptr = 0;
        h->src_valid = false;
    });
}
int fql_replay_add(fql_handle h, const float* ob, const float* ac, float reward, float mask, const float* nob) {
    FQL_ADMIT(h, EP_replay_add);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (h->rb_cap <= 0 || h->visual) throw Invalid{"fql_replay_add: no state replay ring (fql_replay_create; frames agents use fql_replay_add_frames)"};
        if (!ob || !ac || !nob) invalid("transition pointers must not be NULL");
        ring_insert(h, h->rb_obs, h->rb_act, h->rb_rew, h->rb_mask, h->rb_nobs, nullptr, nullptr, h->rb_ptr, ob, ac, reward, mask, nob, nullptr, nullptr);
        h->rb_ptr = (h->rb_ptr + 1) % h->rb_cap;
        h->rb_size = std::max(h->rb_ptr, h->rb_size);
    });
}
int fql_replay_add_frames(fql_handle h, const uint8_t* frame, const uint8_t* next_frame, const float* ac, float reward, float mask) {
    FQL_ADMIT(h, EP_replay_add_frames);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (h->rb_cap <= 0 || !h->visual) throw Invalid{"fql_replay_add_frames: no frames replay ring (fql_replay_create on a frames agent)"};
        if (!frame || !next_frame || !ac) invalid("transition pointers must not be NULL");
        ring_insert(h, nullptr, h->rb_act, h->rb_rew, h->rb_mask, nullptr, h->rb_frames, h->rb_next_frames, h->rb_ptr, nullptr, ac, reward, mask,
                    nullptr, frame, next_frame);
        h->rb_ptr = (h->rb_ptr + 1) % h->rb_cap;
        h->rb_size = std::max(h->rb_ptr, h->rb_size);
    });
}
int fql_replay_size(fql_handle h, int64_t* size, int64_t* pointer) {
    FQL_ADMIT(h, EP_replay_size);
    if (!h) return FQL_E_INVALID;
    if (size) *size = h->rb_size;
    if (pointer) *pointer = h->rb_ptr;
    return FQL_OK;
}
int fql_update_balanced(fql_handle h, const int64_t* idx_dataset, const int64_t* idx_replay, const int32_t* crop_froms, int batch_size,
                        const fql_noise* noise, float* info13, void* stream) {
    FQL_ADMIT(h, EP_update_balanced);
    if (!h) return FQL_E_INVALID;
    if (h->began) { h->err = "fql_update_balanced between fql_update_begin and fql_update_end"; return FQL_E_STATE; }
    return update_with(h, h->prog_full, info13, FQL_NUM_INFO, stream, [&](hipStream_t s) {
        if (h->visual) h->hip_touch();
        h->source_balanced(idx_dataset, idx_replay, crop_froms, batch_size, noise, s);
    });
}

int fql_update_from_dataset_begin(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi,
                                  const fql_noise* noise, void* stream) {
    FQL_ADMIT(h, EP_update_from_dataset_begin);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
        run_program(h, h->prog_fwdbwd, s);
        h->began = true;
        h->split_begun = false;
    });
}
int fql_update_from_dataset_begin_split(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi,
                                        const fql_noise* noise, void* stream0, void* stream1) {
    FQL_ADMIT(h, EP_update_from_dataset_begin_split);
    if (!h) return FQL_E_INVALID;
    if (!h->split_ok || !stream0 || !stream1 || stream0 == stream1) { h->err = "split update unavailable (needs two distinct streams and a two-lane program)"; return FQL_E_STATE; }
    FQL_TRY(h, {
        h->source_from_dataset(idx, batch_size, lo, hi, noise, (hipStream_t)stream0);
        h->launch_split((hipStream_t)stream0, (hipStream_t)stream1);
        h->began = true;
    });
}
int fql_update_begin_split(fql_handle h, const float* obs, const float* act, const float* rew, const float* mask, const float* nobs,
                           int batch_size, const fql_noise* noise, void* stream0, void* stream1) {
    FQL_ADMIT(h, EP_update_begin_split);
    if (!h) return FQL_E_INVALID;
    if (!h->split_ok || !stream0 || !stream1 || stream0 == stream1) { h->err = "split update unavailable (needs two distinct streams and a two-lane program)"; return FQL_E_STATE; }
    FQL_TRY(h, {
        h->source_from_batch(obs, act, rew, mask, nobs, batch_size, noise, 1, (hipStream_t)stream0);
        h->launch_split((hipStream_t)stream0, (hipStream_t)stream1);
        h->began = true;
    });
}
int fql_update_end_split(fql_handle h, float* info13, void* stream0, void* stream1) {
    FQL_ADMIT(h, EP_update_end_split);
    if (!h) return FQL_E_INVALID;
    if (!h->began) { h->err = "fql_update_end_split without fql_update_begin"; return FQL_E_STATE; }
    if (!stream0 || !stream1 || stream0 == stream1) { h->err = "fql_update_end_split needs two distinct streams"; return FQL_E_STATE; }
    FQL_TRY(h, {
        h->run_opt_split((hipStream_t)stream0, (hipStream_t)stream1);
        h->began = false;
        h->finish_info(info13, FQL_NUM_INFO, (hipStream_t)stream0);
    });
}
int fql_grad_buckets(fql_handle h, size_t offsets[2], size_t lengths[2]) {
    FQL_ADMIT(h, EP_grad_buckets);
    if (!h || !offsets || !lengths) return FQL_E_INVALID;
    // bucket 0: both critic members + the BC flow actor (all produced on lane 1); bucket 1: the one-step actor (lane 0's tail)
    offsets[0] = 0; lengths[0] = h->nets[NET_OS].off;
    offsets[1] = h->nets[NET_OS].off; lengths[1] = h->n_train - h->nets[NET_OS].off;
    return h->split_ok ? FQL_OK : FQL_E_STATE;
}
int fql_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                            float* info13, void* stream) {
    FQL_ADMIT(h, EP_update_from_dataset);
    if (h && h->visual) return fql_update_from_frames(h, idx, nullptr, batch_size, lo, hi, noise, info13, stream);
    if (h && !h->began) {
        return update_with(h, h->prog_full, info13, FQL_NUM_INFO, stream, [&](hipStream_t s) {
            h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
        });
    }
    int rc = fql_update_from_dataset_begin(h, idx, batch_size, lo, hi, noise, stream);
    if (rc != FQL_OK) return rc;
    return fql_update_end(h, info13, stream);
}

int fql_info_enqueue(fql_handle h, void* stream, uint64_t* ticket) {
    if (!h || !ticket) return FQL_E_INVALID;
    FQL_TRY_(h, ((h)->group_order(pick(h, stream)), (h)->hip_touch()), {
        hipStream_t s = pick(h, stream);
        const uint64_t k = h->info_seq++;
        const int slot = (int)(k % fql_engine::kInfoRing);
        HIP_CHECK(hipMemcpyAsync(h->h_info_ring[slot], h->info_src(),
                                 std::max(h->num_info(), FQL_NUM_INFO) * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(h->info_ev[slot], s));
        *ticket = k;
    });
}
static int info_wait(fql_handle h, uint64_t ticket, float* info13_host, int n);
int fql_info_wait(fql_handle h, uint64_t ticket, float* info13_host) {
    FQL_ADMIT(h, EP_info_wait);
    return info_wait(h, ticket, info13_host, FQL_NUM_INFO);
}
int fql_info_wait_n(fql_handle h, uint64_t ticket, float* out, int n) {
    if (!h || !out) return FQL_E_INVALID;
    if (n < fql_num_info(h)) { h->err = "fql_info_wait_n: the buffer holds fewer floats than fql_num_info(h)"; return FQL_E_INVALID; }
    return info_wait(h, ticket, out, fql_num_info(h));   // exactly the handle's info count (12 on IFQL / ReBRAC handles)
}
static int info_wait(fql_handle h, uint64_t ticket, float* info13_host, int n) {
    if (!h || !info13_host) return FQL_E_INVALID;
    if (ticket >= h->info_seq) { h->err = "unknown info ticket"; return FQL_E_INVALID; }
    if (h->info_seq - ticket > (uint64_t)fql_engine::kInfoRing) { h->err = "info ticket expired (more than 64 later tickets were taken before it was read)"; return FQL_E_STATE; }
    FQL_TRY(h, {
        const int slot = (int)(ticket % fql_engine::kInfoRing);
        HIP_CHECK(hipEventSynchronize(h->info_ev[slot]));
        std::memcpy(info13_host, h->h_info_ring[slot], n * sizeof(float));
    });
}

int fql_synchronize(fql_handle h, int* mode) {
    if (!h) return FQL_E_INVALID;
    if (mode) *mode = h->last_update_aql ? 1 : 0;
    FQL_TRY(h, {
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->hip_dirty = false;
    });
}

int fql_read_info(fql_handle h, float* info13_host) {
    FQL_ADMIT(h, EP_read_info);
    if (!h || !info13_host) return FQL_E_INVALID;
    FQL_TRY(h, {
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(info13_host, &h->d_state->info[0], FQL_NUM_INFO * sizeof(float), hipMemcpyDeviceToHost));
    });
}
int fql_read_info_n(fql_handle h, float* out, int n) {
    if (!h || !out) return FQL_E_INVALID;
    if (n < fql_num_info(h)) { h->err = "fql_read_info_n: the buffer holds fewer floats than fql_num_info(h)"; return FQL_E_INVALID; }
    FQL_TRY(h, {
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, h->info_src(), (size_t)fql_num_info(h) * sizeof(float), hipMemcpyDeviceToHost));   // exactly fql_num_info(h)
    });
}

// what every *_stats entry point says of an update: the launches of its program and its multiply-accumulates
static void update_stats(const Program& pr, int64_t macs, int64_t* launches_per_update, int64_t* macs_per_update) {
    if (launches_per_update) *launches_per_update = (int64_t)pr.launches.size();
    if (macs_per_update) *macs_per_update = macs;
}
int fql_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update, int64_t* param_count) {
    if (!h) return FQL_E_INVALID;
    update_stats(h->prog_full, h->macs_per_update(), launches_per_update, macs_per_update);
    if (param_count) {
        int64_t n = 0;
        for (const Leaf& l : h->leaves) n += (int64_t)fql_engine::leaf_count(l);
        *param_count = n;
    }
    return FQL_OK;
}
void* fql_stream(fql_handle h) { return h ? (void*)h->stream : nullptr; }

// ---- ReBRAC (agents/rebrac.py) ---------------------------------------------------------------------------------------------------
// One update: the full program (full_update != 0) or the critic-only one, through run_update (the AQL form and the graph are bitwise equal).
int fql_rebrac_update(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                      const float* next_actions, int batch_size, const fql_noise* noise, int full_update, float* info13, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_rebrac_update);
    return update_with(h, full_update ? h->prog_full : h->prog_critic, info13, FQL_NUM_INFO, stream, [&](hipStream_t s) {
        h->rebrac_source_from_batch(obs, act, rew, masks, next_obs, next_actions, batch_size, noise, 1, s);
    });
}
int fql_rebrac_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                   int full_update, float* info13, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_rebrac_update_from_dataset);
    return update_with(h, full_update ? h->prog_full : h->prog_critic, info13, FQL_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
    });
}
int fql_rebrac_total_loss(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                          const float* next_actions, int batch_size, const fql_noise* noise, int full_update, float* loss, float* info10,
                          void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_rebrac_total_loss);
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->rebrac_source_from_batch(obs, act, rew, masks, next_obs, next_actions, batch_size, noise, 0, s);
        run_program(h, h->prog_loss, s);
        float tmp[9];
        HIP_CHECK(hipMemcpyAsync(tmp, &h->d_state->info[0], sizeof tmp, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // rebrac.py:86-108: critic_loss (+ the actor's total_loss on a full step); 9 infos, or the 4 critic ones
        if (loss) *loss = full_update ? tmp[0] + tmp[4] : tmp[0];
        if (info10) std::memcpy(info10, tmp, (full_update ? 9 : 4) * sizeof(float));
    });
}
int fql_rebrac_sample_actions(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, float temperature, float* out,
                              void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_rebrac_sample_actions);
    FQL_TRY(h, h->sample(obs, noise, seed, temperature, n, out, pick(h, stream), stream == nullptr));
}
int fql_rebrac_stats(fql_handle h, int full_update, int64_t* launches_per_update, int64_t* macs_per_update) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_rebrac_stats);
    update_stats(full_update ? h->prog_full : h->prog_critic, h->rebrac_macs(full_update != 0), launches_per_update, macs_per_update);
    return FQL_OK;
}

// ---- SAC (agents/sac.py; RLPD = SAC online with balanced sampling) ----------------------------------------------------------------
// One update through run_update (the AQL form and the graph are bitwise equal); 14 infos.
int fql_sac_update(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                   int batch_size, const fql_noise* noise, float* info14, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sac_update);
    return update_with(h, h->prog_full, info14, FQL_SAC_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_from_batch(obs, act, rew, masks, next_obs, batch_size, noise, 1, s);
    });
}
int fql_sac_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                float* info14, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sac_update_from_dataset);
    return update_with(h, h->prog_full, info14, FQL_SAC_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
    });
}
int fql_sac_update_balanced(fql_handle h, const int64_t* idx_dataset, const int64_t* idx_replay, int batch_size, const fql_noise* noise,
                            float* info14, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sac_update_balanced);
    return update_with(h, h->prog_full, info14, FQL_SAC_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_balanced(idx_dataset, idx_replay, nullptr, batch_size, noise, s);
    });
}
int fql_sac_total_loss(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                       int batch_size, const fql_noise* noise, float* loss, float* info11, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sac_total_loss);
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->source_from_batch(obs, act, rew, masks, next_obs, batch_size, noise, 0, s);
        // the probe writes info slots 0-10 and 14: keep the last update's infos (fql_read_info_n after the probe still reads them)
        float keep[16], tmp[SAC_I_Q + 1];
        HIP_CHECK(hipMemcpyAsync(keep, &h->d_state->info[0], sizeof keep, hipMemcpyDeviceToHost, s));
        run_program(h, h->prog_loss, s);
        HIP_CHECK(hipMemcpyAsync(tmp, &h->d_state->info[0], sizeof tmp, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&h->d_state->info[0], keep, sizeof keep, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        tmp[10] = tmp[SAC_I_Q];   // actor/q (scratch slot while no finalize runs)
        // sac.py:94-112: loss = critic_loss + the actor's total_loss; infos 0-10
        if (loss) *loss = tmp[0] + tmp[4];
        if (info11) std::memcpy(info11, tmp, 11 * sizeof(float));
    });
}
int fql_sac_sample_actions(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, float temperature, float* out,
                           void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sac_sample_actions);
    FQL_TRY(h, h->sample(obs, noise, seed, temperature, n, out, pick(h, stream), stream == nullptr));
}
int fql_sac_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sac_stats);
    update_stats(h->prog_full, h->macs_per_update(), launches_per_update, macs_per_update);
    return FQL_OK;
}

// ---- IQL (agents/iql.py): expectile value, Gaussian actor with the AWR or the DDPG+BC loss -------------------------------------------
// One update through run_update (the AQL form and the graph are bitwise equal); 16 (awr) or 19 (ddpgbc) infos.
void fql_iql_default_config(fql_iql_config* c) {   // agents/iql.py:242-261
    std::memset(c, 0, sizeof *c);
    c->expectile = 0.9f;
    c->alpha = 1.0f;
    c->actor_loss = 1;
    c->const_std = 1;
}
int fql_iql_create(const fql_config* cfg, const fql_iql_config* qcfg, uint64_t seed, fql_handle* out) {
    if (!qcfg) { g_create_error = "qcfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::IQL, qcfg}, seed, out);
}
int fql_iql_update(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                   int batch_size, const fql_noise* noise, float* info, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iql_update);
    return update_with(h, h->prog_full, info, h->num_info(), stream, [&](hipStream_t s) {
        h->source_from_batch(obs, act, rew, masks, next_obs, batch_size, noise, 1, s);
    });
}
int fql_iql_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                float* info, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iql_update_from_dataset);
    return update_with(h, h->prog_full, info, h->num_info(), stream, [&](hipStream_t s) {
        h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
    });
}
int fql_iql_total_loss(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                       int batch_size, const fql_noise* noise, float* loss, float* info, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iql_total_loss);
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->source_from_batch(obs, act, rew, masks, next_obs, batch_size, noise, 0, s);
        run_program(h, h->prog_loss, s);   // its finalize writes the probe half of iql_info: the last update's infos stay
        float tmp[IQL_INFO_STRIDE];
        HIP_CHECK(hipMemcpyAsync(tmp, h->iql_info + IQL_INFO_STRIDE, sizeof tmp, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // iql.py:115-134: loss = value_loss + critic_loss + actor_loss; every info but the grad statistics
        if (loss) *loss = tmp[0] + tmp[4] + tmp[IQL_I_ACTOR];
        if (info) std::memcpy(info, tmp, (size_t)(fql_num_info(h) - 3) * sizeof(float));
    });
}
int fql_iql_sample_actions(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, float temperature, float* out,
                           void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iql_sample_actions);
    FQL_TRY(h, h->sample(obs, noise, seed, temperature, n, out, pick(h, stream), stream == nullptr));
}
int fql_iql_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iql_stats);
    update_stats(h->prog_full, h->macs_per_update(), launches_per_update, macs_per_update);
    return FQL_OK;
}

// ---- BC (agents/bc.py): flow-matching behavioural cloning -------------------------------------------------------------------------
// One update through run_update (the AQL form and the graph are bitwise equal); 4 infos.
void fql_bc_default_config(fql_bc_config* c) {   // agents/bc.py:135-148
    std::memset(c, 0, sizeof *c);
    c->denoise_steps = 16;
}
int fql_bc_create(const fql_config* cfg, const fql_bc_config* bcfg, uint64_t seed, fql_handle* out) {
    if (!bcfg) { g_create_error = "bcfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::BC, bcfg}, seed, out);
}
int fql_bc_update(fql_handle h, const float* obs, const float* act, int batch_size, const fql_noise* noise, float* info4, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_bc_update);
    return update_with(h, h->prog_full, info4, FQL_BC_NUM_INFO, stream, [&](hipStream_t s) {
        h->bc_source_from_batch(obs, act, batch_size, noise, 1, s);
    });
}
int fql_bc_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                               float* info4, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_bc_update_from_dataset);
    return update_with(h, h->prog_full, info4, FQL_BC_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
    });
}
int fql_bc_policy_loss(fql_handle h, const float* obs, const float* act, int batch_size, const fql_noise* noise, float* loss, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_bc_policy_loss);
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->bc_source_from_batch(obs, act, batch_size, noise, 0, s);
        run_program(h, h->prog_loss, s);   // writes info slot 5 only: the four slots fql_read_info_n reads stay the last update's
        float v = 0.f;
        HIP_CHECK(hipMemcpyAsync(&v, &h->d_state->info[BC_I_LOSS], sizeof v, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (loss) *loss = v;
    });
}
int fql_bc_sample_actions(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, float* out, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_bc_sample_actions);
    FQL_TRY(h, h->sample(obs, noise, seed, 1.0f, n, out, pick(h, stream), stream == nullptr));
}
int fql_bc_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update, int64_t* launches_per_sample) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_bc_stats);
    FQL_TRY(h, {
        update_stats(h->prog_full, h->macs_per_update(), launches_per_update, macs_per_update);
        if (launches_per_sample) *launches_per_sample = h->sample_flow_launches(false);   // assemble, step-bias table, C0, S (layer 0 + nh GEMMs), extract
    });
}

// ---- IQL-diffusion (agents/iql_diffusion.py): IQL critics, weighted flow actor, classifier-free guidance -----------------------------
// One update through run_update (the AQL form and the graph are bitwise equal), one program per step kind; 21 infos.
static_assert(IQLD_NUM_INFO == FQL_IQLD_NUM_INFO && IQLD_INFO_STRIDE == IQL_INFO_STRIDE, "IQL-diffusion info layout");
void fql_iqld_default_config(fql_iqld_config* c) {   // agents/iql_diffusion.py:362-396
    std::memset(c, 0, sizeof *c);
    c->actor_lr = c->value_lr = c->critic_lr = 3e-4f;
    c->expectile = 0.9f;
    c->awr_temperature = 0.1f;
    c->softmax_beta = 3.0f;
    c->optimal_var = IQLD_BINARY_AWR;
    c->target_extraction = 1;
    c->denoise_steps = 16;
    c->opt_decay_schedule = 0;
}
int fql_iqld_create(const fql_config* cfg, const fql_iqld_config* dcfg, uint64_t seed, fql_handle* out) {
    if (!dcfg) { g_create_error = "dcfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::IQLD, dcfg}, seed, out);
}
int fql_iqld_update(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                    int batch_size, const fql_noise* noise, int update_critic, int update_actor, float* info, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_update);
    return update_with(h, h->iqld_program(update_critic != 0, update_actor != 0), info, FQL_IQLD_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_from_batch(obs, act, rew, masks, next_obs, batch_size, noise, 1, s);
    });
}
int fql_iqld_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                 int update_critic, int update_actor, float* info, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_update_from_dataset);
    return update_with(h, h->iqld_program(update_critic != 0, update_actor != 0), info, FQL_IQLD_NUM_INFO, stream, [&](hipStream_t s) {
        h->source_from_dataset(idx, batch_size, lo, hi, noise, s);
    });
}
int fql_iqld_total_loss(fql_handle h, const float* obs, const float* act, const float* rew, const float* masks, const float* next_obs,
                        int batch_size, const fql_noise* noise, float* loss, float* info, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_total_loss);
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->source_from_batch(obs, act, rew, masks, next_obs, batch_size, noise, 0, s);
        run_program(h, h->prog_loss, s);   // writes the probe halves of the info and row buffers: the last update's stay
        float tmp[IQLD_INFO_STRIDE];
        HIP_CHECK(hipMemcpyAsync(tmp, h->iql_info + IQLD_INFO_STRIDE, sizeof tmp, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // iql_diffusion.py:272-285: critic_loss + value_loss + actor_loss; every info but the grad statistics
        if (loss) *loss = tmp[IQLD_I_CRITIC] + tmp[IQLD_I_VALUE] + tmp[IQLD_I_ACTOR + 1];
        if (info) std::memcpy(info, tmp, (size_t)IQLD_I_GRAD * sizeof(float));
    });
}
int fql_iqld_sample_actions(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, float cfg, float* out, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_sample_actions);
    FQL_TRY(h, h->sample_flow(obs, noise, seed, n, out, pick(h, stream), stream == nullptr, {nullptr, cfg}));
}
int fql_iqld_read_rows(fql_handle h, int which, float* out, int n) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_read_rows);
    FQL_TRY(h, {
        if (which < 0 || which > 5) invalid("which must be in [0, 5] (got %d)", which);
        if (!out) invalid("out must not be NULL");
        if (n != h->B) invalid("n = %d does not match the batch size %d", n, h->B);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, h->rows_buf + (size_t)which * h->B, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    });
}
int fql_iqld_get_steps(fql_handle h, int64_t steps[3]) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_get_steps);
    FQL_TRY(h, {
        if (!steps) invalid("steps must not be NULL");
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipDeviceSynchronize());
        DevState st, sa;
        HIP_CHECK(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&sa, h->d_state_a, sizeof sa, hipMemcpyDeviceToHost));
        steps[0] = (int64_t)st.rng_step; steps[1] = st.adam_count; steps[2] = sa.adam_count;
    });
}
int fql_iqld_set_steps(fql_handle h, const int64_t steps[3]) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_set_steps);
    FQL_TRY(h, {
        if (!steps) invalid("steps must not be NULL");
        if (steps[0] < 0 || steps[1] < 0 || steps[2] < 0) invalid("the counters must be >= 0");
        HIP_CHECK(hipDeviceSynchronize());
        DevState st, sa;
        HIP_CHECK(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&sa, h->d_state_a, sizeof sa, hipMemcpyDeviceToHost));
        st.rng_step = (uint64_t)steps[0];
        st.adam_count = steps[1]; st.train_step = steps[1] + 1;
        st.b1pow = std::pow(0.9, (double)steps[1]); st.b2pow = std::pow(0.999, (double)steps[1]);
        sa.adam_count = steps[2]; sa.train_step = steps[2] + 1;
        sa.b1pow = std::pow(0.9, (double)steps[2]); sa.b2pow = std::pow(0.999, (double)steps[2]);
        HIP_CHECK(hipMemcpy(h->d_state, &st, sizeof st, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(h->d_state_a, &sa, sizeof sa, hipMemcpyHostToDevice));
    });
}
int fql_iqld_stats(fql_handle h, int update_critic, int update_actor, int64_t* launches_per_update, int64_t* macs_per_update,
                   int64_t* launches_per_sample) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_stats);
    FQL_TRY(h, {
        update_stats(h->iqld_program(update_critic != 0, update_actor != 0), h->iqld_macs(update_critic != 0, update_actor != 0), launches_per_update, macs_per_update);
        // assemble, step-bias table, C0, S (layer 0 + nh GEMMs + the CFG step), extract
        if (launches_per_sample) *launches_per_sample = h->sample_flow_launches(false);
    });
}

// ---- CFGRL (agents/cfgrl.py): goal-conditioned flow policy, classifier-free guidance -------------------------------------------------
// One update through run_update (the AQL form and the graph are bitwise equal); 4 infos.
static_assert(FQL_CFGRL_NUM_INFO == 4, "CFGRL info layout");
void fql_cfgrl_default_config(fql_cfgrl_config* c) {   // agents/cfgrl.py:162-191
    std::memset(c, 0, sizeof *c);
    c->goal_dim = 0;
    c->flow_steps = 16;
    c->cfg = 3.0f;
    c->p_uncond = 0.1;
    c->actor_p_curgoal = 0.0; c->actor_p_trajgoal = 1.0; c->actor_p_randomgoal = 0.0;
    c->actor_geom_sample = 0;
}
int fql_cfgrl_create(const fql_config* cfg, const fql_cfgrl_config* gcfg, uint64_t seed, fql_handle* out) {
    if (!gcfg) { g_create_error = "gcfg must not be NULL"; if (out) *out = nullptr; return FQL_E_INVALID; }
    return create_engine(cfg, {AgentKind::CFGRL, gcfg}, seed, out);
}
int fql_cfgrl_update(fql_handle h, const float* obs, const float* act, const float* goals, int batch_size, const fql_noise* noise,
                     const uint8_t* do_cfg, float* info4, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_update);
    return update_with(h, h->prog_full, info4, FQL_CFGRL_NUM_INFO, stream, [&](hipStream_t s) {
        h->cfgrl_source_from_batch(obs, act, goals, do_cfg, batch_size, noise, 1, s);
    });
}
int fql_cfgrl_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                  const uint8_t* do_cfg, float* info4, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_update_from_dataset);
    return update_with(h, h->prog_full, info4, FQL_CFGRL_NUM_INFO, stream, [&](hipStream_t s) {
        h->cfgrl_source_from_dataset(idx, batch_size, lo, hi, noise, do_cfg, s);
    });
}
int fql_cfgrl_policy_loss(fql_handle h, const float* obs, const float* act, const float* goals, int batch_size, const fql_noise* noise,
                          const uint8_t* do_cfg, float* loss, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_policy_loss);
    FQL_TRY(h, {
        hipStream_t s = pick(h, stream);
        h->cfgrl_source_from_batch(obs, act, goals, do_cfg, batch_size, noise, 0, s);
        run_program(h, h->prog_loss, s);   // writes info slot 5 and the probe half of the row read-back: what fql_read_info_n reads stays the last update's
        float v = 0.f;
        HIP_CHECK(hipMemcpyAsync(&v, &h->d_state->info[CFGRL_I_LOSS], sizeof v, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (loss) *loss = v;
    });
}
int fql_cfgrl_dataset_goals(fql_handle h, const int64_t* final_idx, const float* reps) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_dataset_goals);
    FQL_TRY(h, {
        const int64_t n = h->ds_size;
        const int Gd = h->gcfg.goal_dim;
        if (!h->ds_obs || n <= 0) throw Invalid{"fql_cfgrl_dataset_goals: no dataset uploaded (fql_dataset_upload)"};
        if (n >= ((int64_t)1 << 32)) invalid("fql_cfgrl_dataset_goals: %lld rows: the goal draw indexes fewer than 2^32", (long long)n);
        if (!final_idx) invalid("final_idx must not be NULL");
        if (!reps && Gd != h->cfg.obs_dim) invalid("goal_dim %d differs from obs_dim %d: pass the [N, %d] representations", Gd, h->cfg.obs_dim, Gd);
        if (!fql_engine::is_device_ptr(final_idx))   // the device reads row final_idx[i] of the representations: every entry must name a row at or behind i
            for (int64_t i = 0; i < n; ++i)
                if (final_idx[i] < i || final_idx[i] >= n) invalid("final_idx[%lld] = %lld is not in [%lld, %lld)", (long long)i, (long long)final_idx[i], (long long)i, (long long)n);
        HIP_CHECK(hipDeviceSynchronize());
        h->drop_goal_table();
        HIP_CHECK(hipMalloc((void**)&h->ds_final, (size_t)n * sizeof(int64_t)));
        HIP_CHECK(hipMemcpy(h->ds_final, final_idx, (size_t)n * sizeof(int64_t), hipMemcpyDefault));
        if (reps) {
            HIP_CHECK(hipMalloc((void**)&h->ds_reps, (size_t)n * Gd * sizeof(float)));
            HIP_CHECK(hipMemcpy(h->ds_reps, reps, (size_t)n * Gd * sizeof(float), hipMemcpyDefault));
        }
        h->gsrc_valid = false;
    });
}
int fql_cfgrl_sample_actions(fql_handle h, const float* obs, const float* goals, int n, const float* noise, uint64_t seed, float cfg,
                             float* out, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_sample_actions);
    FQL_TRY(h, h->sample_flow(obs, noise, seed, n, out, pick(h, stream), stream == nullptr, {goals, cfg}));
}
int fql_cfgrl_read_rows(fql_handle h, int probe, int64_t* idx, int64_t* goal_idx, uint8_t* do_cfg, uint32_t* draws, float* goals, int n) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_read_rows);
    FQL_TRY(h, {
        if (probe != 0 && probe != 1) invalid("probe must be 0 (the last update) or 1 (the last policy_loss)");
        if (n != h->B) invalid("n = %d does not match the batch size %d", n, h->B);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipDeviceSynchronize());
        const size_t B = (size_t)h->B;
        const int64_t* rows = h->cf_rows + (size_t)probe * 2 * B;
        if (idx) HIP_CHECK(hipMemcpy(idx, rows, B * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (goal_idx) HIP_CHECK(hipMemcpy(goal_idx, rows + B, B * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (do_cfg) HIP_CHECK(hipMemcpy(do_cfg, h->cf_mask + (size_t)probe * B, B, hipMemcpyDeviceToHost));
        if (draws) HIP_CHECK(hipMemcpy(draws, h->cf_draws + (size_t)probe * CFGRL_NUM_DRAWS * B, CFGRL_NUM_DRAWS * B * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (goals) {   // the goal columns of the assembled input rows (the probe shares X with the update: the rows of whichever ran last)
            const int Gd = h->gcfg.goal_dim, inp = h->nets[NET_BC].in_p();
            HIP_CHECK(hipMemcpy2D(goals, (size_t)Gd * sizeof(float), h->X_bc + h->cfg.obs_dim, (size_t)inp * sizeof(float), (size_t)Gd * sizeof(float), B,
                                  hipMemcpyDeviceToHost));
        }
    });
}
int fql_cfgrl_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update, int64_t* launches_per_sample) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_stats);
    FQL_TRY(h, {
        update_stats(h->prog_full, h->macs_per_update(), launches_per_update, macs_per_update);
        // assemble, C0, S (layer 0 + nh GEMMs + the CFG step), extract
        if (launches_per_sample) *launches_per_sample = h->sample_flow_launches(false);
    });
}

// ---- guidance sweeps: the two CFG samplers with one weight per row ------------------------------------------
int fql_iqld_sample_actions_cfgs(fql_handle h, const float* obs, int n, const float* noise, uint64_t seed, const float* cfgs, float* out,
                                 void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_iqld_sample_actions_cfgs);
    FQL_TRY(h, h->sample_flow(obs, noise, seed, n, out, pick(h, stream), stream == nullptr, {nullptr, 1.0f, cfgs, true}));
}
int fql_cfgrl_sample_actions_cfgs(fql_handle h, const float* obs, const float* goals, int n, const float* noise, uint64_t seed,
                                  const float* cfgs, float* out, void* stream) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_cfgrl_sample_actions_cfgs);
    FQL_TRY(h, h->sample_flow(obs, noise, seed, n, out, pick(h, stream), stream == nullptr, {goals, 1.0f, cfgs, true}));
}
int fql_sample_cfgs_stats(fql_handle h, int64_t* launches_per_call) {
    if (!h) return FQL_E_INVALID;
    FQL_ADMIT(h, EP_sample_cfgs_stats);
    FQL_TRY(h, {
        const int64_t n = h->sample_flow_launches(true);
        if (launches_per_call) *launches_per_call = n;
    });
}

}  // extern "C"

// Per-launch device times of ONE update, measured with HIP events on the engine's stream (used by bench.py for the per-kernel
// roofline: rocprofv3 serialises the graph's lanes, and so does this pass - the launches run eagerly, in program order, on one
// stream, an event before and after each).  It IS a real update (state advances).  Needs a device-resident dataset.
// Out, per launch (up to cap): op type (OpType), lane, workgroups, microseconds, algorithmic MACs of its GEMM-shaped tasks.
// An event-to-event interval holds the launch gap in front of the kernel besides the kernel: *null_us receives the same interval for a
// one-workgroup kernel that returns at once (median of 32), which the caller subtracts (minus the ~1.4 us such a kernel itself shows
// in a rocprofv3 trace) to compare with rocprofv3's per-kernel durations.
extern "C" int fql_profile_update(fql_handle h, int batch_size, int cap, int* type, int* lane, int* grid, float* us, double* macs, float* null_us) {
    FQL_ADMIT(h, EP_profile_update);
    if (!h || !type || !us) return FQL_E_INVALID;
    try {
        require_graph(h->prog_full);
        hipStream_t s = h->stream;
        if (null_us) *null_us = 0.f;   // (no calibration needed: the events ride on the dispatches)
        h->source_from_dataset(nullptr, batch_size, 0, 0, nullptr, s);
        Program& pr = h->prog_full;
        const int n = (int)pr.launches.size();
        std::vector<hipEvent_t> ev(2 * n);
        for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
        for (int i = 0; i < n; ++i) {   // the update's launches in program order on one stream, each dispatch carrying its own event pair
            h->prof_a = ev[2 * i]; h->prof_b = ev[2 * i + 1];
            h->issue(pr.launches[i], s, -1);
        }
        h->prof_a = h->prof_b = nullptr;
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < n && i < cap; ++i) {
            const Launch& L = pr.launches[i];
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            type[i] = (int)L.type; if (lane) lane[i] = L.lane; if (grid) grid[i] = L.grid; us[i] = ms * 1e3f;
            if (macs) macs[i] = L.macs;
        }
        for (auto& e : ev) hipEventDestroy(e);
        return std::min(n, cap);
    } catch (const Invalid& e) { h->prof_a = h->prof_b = nullptr; h->err = e.msg; return FQL_E_INVALID; }
    catch (const HipError& e) { h->prof_a = h->prof_b = nullptr; h->err = e.msg; return FQL_E_HIP; }
}

// Diagnostic only (not in include/fql_amd.h): copy a workspace buffer of the last update to the host, so tests can look at what the
// production RNG / gather path actually produced.  which: 0 X_os [3B, inp_c], 1 X_bc [B, inp_b], 2 vel [B, ap], 3 w_act [B, ap],
// 4 X_c1 [B, inp_c], 5 w_rew [B], 6 w_mask [B], 7 in_idx (int64 [B], frames path), 8 in_crop (int32 [B][2], frames path),
// 9 X_eu [B, inp_b].  *dims receives {rows, row stride in elements}.
extern "C" int fql_debug_workspace(fql_handle h, int which, void* out, size_t bytes, int* dims) {
    FQL_ADMIT(h, EP_debug_workspace);
    if (!h || !out) return FQL_E_INVALID;
    const int B = h->B, ic = h->nets[NET_OS].in_p(), ib = h->nets[NET_BC].in_p(), ap = pad16(h->cfg.act_dim);
    const void* src = nullptr;
    size_t n = 0, esz = sizeof(float);
    int rows = B, ld = 1;
    switch (which) {
        case 0: src = h->X_os; rows = 3 * B; ld = ic; break;
        case 1: src = h->X_bc; ld = ib; break;
        case 2: src = h->vel; ld = ap; break;
        case 3: src = h->w_act; ld = ap; break;
        case 4: src = h->X_c1; ld = ic; break;
        case 5: src = h->w_rew; break;
        case 6: src = h->w_mask; break;
        case 7: src = h->in_idx; esz = sizeof(int64_t); break;
        case 8: src = h->in_crop; esz = sizeof(int); ld = 2; break;
        case 9: src = h->X_eu; ld = ib; break;
        default: return FQL_E_INVALID;
    }
    if (!src) return FQL_E_NOTFOUND;
    n = (size_t)rows * ld * esz;
    if (dims) { dims[0] = rows; dims[1] = ld; }
    if (bytes < n) return FQL_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return FQL_E_HIP;
    return hipMemcpy(out, src, n, hipMemcpyDeviceToHost) == hipSuccess ? FQL_OK : FQL_E_HIP;
}

// Diagnostic only (not in include/fql_amd.h), -DFQL_TIMELINE builds: per launch of the single-graph update (prog_full) lane, op type,
// grid and the device wall-clock times (us, relative to the first entry) of its first / last workgroup entry and last exit.
// reset = 1 clears the table (call before the update to be examined).  Returns the number of launches, or < 0.
extern "C" int fql_debug_timeline(fql_handle h, int reset, int cap, int* lane, int* type, int* grid, double* t_first, double* t_last, double* t_exit) {
#ifdef FQL_TIMELINE
    if (!h) return FQL_E_INVALID;
    try { h->aql_drain(); } catch (...) { return FQL_E_HIP; }
    hipDeviceSynchronize();
    static std::vector<unsigned long long> host((size_t)FQL_TL_MAX * FQL_TL_WGS * 2);
    // updates dispatched as AQL packets run the engine's OWN copy of the code object: its instance of the table, not the one HIP registered
    void* aql_tab = nullptr;
    if (h->aql.up && h->last_update_aql) {
        hsa_executable_symbol_t sym;
        if (hsa_executable_get_symbol_by_name(h->aql.exe, "g_fql_tl", &h->aql.agent, &sym) == HSA_STATUS_SUCCESS) {
            uint64_t addr = 0;
            if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_VARIABLE_ADDRESS, &addr) == HSA_STATUS_SUCCESS) aql_tab = (void*)(uintptr_t)addr;
        }
    }
    if (reset) {
        std::fill(host.begin(), host.end(), 0ull);
        if (h->aql.up) {   // both instances
            hsa_executable_symbol_t sym;
            uint64_t addr = 0;
            if (hsa_executable_get_symbol_by_name(h->aql.exe, "g_fql_tl", &h->aql.agent, &sym) == HSA_STATUS_SUCCESS &&
                hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_VARIABLE_ADDRESS, &addr) == HSA_STATUS_SUCCESS && addr)
                if (hipMemcpy((void*)(uintptr_t)addr, host.data(), host.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return FQL_E_HIP;
        }
        return hipMemcpyToSymbol(HIP_SYMBOL(g_fql_tl), host.data(), host.size() * 8) == hipSuccess ? 0 : FQL_E_HIP;
    }
    if (aql_tab) { if (hipMemcpy(host.data(), aql_tab, host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return FQL_E_HIP; }
    else if (hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(g_fql_tl), host.size() * 8) != hipSuccess) return FQL_E_HIP;
    const int n = std::min<int>((int)h->prog_full.launches.size(), std::min(cap, FQL_TL_MAX));
    unsigned long long t0 = ~0ull;
    std::vector<unsigned long long> a(n, ~0ull), b(n, 0), c(n, 0);
    for (int i = 0; i < n; ++i) {
        grid[i] = 0;
        for (int w = 0; w < FQL_TL_WGS; ++w) {
            const unsigned long long e = host[((size_t)i * FQL_TL_WGS + w) * 2], x = host[((size_t)i * FQL_TL_WGS + w) * 2 + 1];
            if (!e) continue;
            grid[i]++;
            a[i] = std::min(a[i], e); b[i] = std::max(b[i], e); c[i] = std::max(c[i], x);
        }
        if (grid[i]) t0 = std::min(t0, a[i]);
    }
    for (int i = 0; i < n; ++i) {
        const Launch& L = h->prog_full.launches[i];
        lane[i] = L.lane; type[i] = (int)L.type;
        t_first[i] = grid[i] ? (double)(a[i] - t0) / 100.0 : -1.0;
        t_last[i] = grid[i] ? (double)(b[i] - t0) / 100.0 : -1.0;
        t_exit[i] = c[i] ? (double)(c[i] - t0) / 100.0 : -1.0;
    }
    return n;
#else
    (void)h; (void)reset; (void)cap; (void)lane; (void)type; (void)grid; (void)t_first; (void)t_last; (void)t_exit;
    return FQL_E_STATE;
#endif
}

// Diagnostic only (not in include/fql_amd.h): copy an encoder-pass buffer to the host.  enc: 0 critic, 1 bc_flow, 2 onestep, 3 target;
// code: 100 s + {0: c0, 1: pool, 10 k + 2: c1[k], 10 k + 3: y[k], 4: arg (bytes)}, 900: frelu, 901: z, 902: E, 903: dz, 904: dA, 905: dB, 906: dC;
// 100 s + 50: stack s's plan as int32 [pool_fused, then per convolution j: split, R forward, R data gradient, R weight gradient]
// (split: the layer runs bf16 x 3; R: image rows per workgroup that conv_rows chose; 0 where that form never runs).
// A request larger than the buffer is refused (FQL_E_INVALID); an unknown code is FQL_E_NOTFOUND.
extern "C" int fql_debug_enc(fql_handle h, int enc, int code, void* out, size_t bytes) {
    if (!h || !h->visual || enc < 0 || enc >= NUM_ENC || code < 0 || (bytes && !out)) return FQL_E_INVALID;
    EncBuf* b = enc == 0 ? &h->eb_c : enc == 1 ? &h->eb_bc : enc == 2 ? &h->eb_os : &h->eb_t;
    const void* src = nullptr;
    if (code >= 900) {
        const void* tab[] = {b->frelu, b->z, b->E, b->dz, b->dA, b->dB, b->dC};
        if (code - 900 < 7) src = tab[code - 900];
    } else if ((size_t)(code / 100) < b->st.size()) {
        const int si = code / 100, k = code % 100;
        EncBuf::St& s = b->st[si];
        if (k == 50) {   // the plan: computed on the host, no device copy
            const EncStack& st = h->encs[enc].stacks[si];
            std::vector<int32_t> plan{st.conv[0].pool_fused ? 1 : 0};
            for (size_t j = 0; j < st.conv.size(); ++j) {
                const ConvL& c = st.conv[j];
                const int H = j == 0 ? st.H : st.H / 2, W = j == 0 ? st.W : st.W / 2, Ci = pad16c(c.cin);
                const bool u8 = si == 0 && j == 0;
                plan.push_back(u8 ? (h->cfg.precision == 2 ? 1 : 0) : (c.split ? 1 : 0));
                plan.push_back(fql_engine::conv_rows(H, W, Ci, c.cout, false));
                plan.push_back(u8 ? 0 : fql_engine::conv_rows(H, W, c.cout, Ci, false));
                plan.push_back(fql_engine::conv_rows(H, W, Ci, c.cout, true, u8));
            }
            if (bytes > plan.size() * sizeof(int32_t)) return FQL_E_INVALID;
            std::memcpy(out, plan.data(), bytes);
            return FQL_OK;
        }
        if (k == 0) src = s.c0;
        else if (k == 1) src = s.pool;
        else if (k == 4) src = s.arg;
        else if (k % 10 == 2 && (size_t)(k / 10) < s.c1.size()) src = s.c1[k / 10];
        else if (k % 10 == 3 && (size_t)(k / 10) < s.y.size()) src = s.y[k / 10];
    }
    if (!src) return FQL_E_NOTFOUND;
    auto it = b->bytes.find(src);
    if (it == b->bytes.end() || bytes > it->second) return FQL_E_INVALID;
    hipDeviceSynchronize();
    return hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? FQL_OK : FQL_E_HIP;
}

// Diagnostic only (not in include/fql_amd.h): what the update program (prog_full) of a state agent will launch, as int32 words.  Nothing is
// launched and no state changes: the launches are what schedule() and the emit sites bound (Launch::k, what issue() hands to the runtime), the tasks
// from the host copies of the tables schedule() uploaded.  Layout:
//   [words in the plan (this one included), launches], then per launch
//   [index, lane, op type, grid (workgroups), kernel entry, GEMM tasks g, weight-gradient tasks w, LayerNorm-backward tasks l, chain records c (0 / 1)]
//   g x [M, N, K, rows per tile, column tiles per wave (wk), xg]     w x [M, Kin, N, split body (0 / 1)]     l x [M]
//   c x [M, H, variant, xg, split (0 / 1)]
// kernel entry: 0 = the launch's only kernel, named by its op type; 1 / 2 fql_gemm16_kernel<false / true>; 3 / 4 fql_gemm16_euler_kernel<false / true>;
// 5 fql_side_kernel; 6 fql_side_split_kernel; 7 fql_side_big_kernel; 8 fql_chain_kernel<H, variant>; 9 fql_chain_split_kernel<H, variant> - found by
// the address of the recorded kernel, so H, variant and `split` of a chain record are those of the instantiation dispatched, and M and xg are read from
// the ChainArgs recorded with it.  Rows per tile: 16 in an OP_GEMM launch, 32 tmt in an OP_GEMM64 launch.
// The first `bytes` bytes of the plan are copied out (4 bytes give its size): a request larger than the plan is FQL_E_INVALID.  Refused with
// FQL_E_STATE: a visual handle (its update is led by HIP launches that are not in prog_full), and a handle that holds no update program (the last
// fql_set_batch_size failed halfway).  Every agent kind builds a prog_full, so no kind is refused.
namespace {
enum { PLAN_K_OTHER = 0, PLAN_K_GEMM16, PLAN_K_GEMM16_KBIG, PLAN_K_GEMM16_EULER, PLAN_K_GEMM16_EULER_KBIG, PLAN_K_SIDE, PLAN_K_SIDE_SPLIT, PLAN_K_SIDE_BIG,
       PLAN_K_CHAIN, PLAN_K_CHAIN_SPLIT };
struct PlanKernel { const void* fn; int entry, H, V; };
template <typename... Pm> const void* plan_fn(void (*k)(Pm...)) { return (const void*)k; }   // the address a launch binds (Bound::fn)
const std::vector<PlanKernel>& plan_kernels() {
#define FQL_PLAN_CHAIN(HH) \
    {plan_fn(fql_chain_kernel<HH, 0>), PLAN_K_CHAIN, HH, 0}, {plan_fn(fql_chain_kernel<HH, 1>), PLAN_K_CHAIN, HH, 1},                    \
    {plan_fn(fql_chain_kernel<HH, 2>), PLAN_K_CHAIN, HH, 2}, {plan_fn(fql_chain_kernel<HH, 3>), PLAN_K_CHAIN, HH, 3},                    \
    {plan_fn(fql_chain_split_kernel<HH, 0>), PLAN_K_CHAIN_SPLIT, HH, 0}, {plan_fn(fql_chain_split_kernel<HH, 1>), PLAN_K_CHAIN_SPLIT, HH, 1}, \
    {plan_fn(fql_chain_split_kernel<HH, 2>), PLAN_K_CHAIN_SPLIT, HH, 2}
    static const std::vector<PlanKernel> t = {
        {plan_fn(fql_gemm16_kernel<false>), PLAN_K_GEMM16, 0, 0}, {plan_fn(fql_gemm16_kernel<true>), PLAN_K_GEMM16_KBIG, 0, 0},
        {plan_fn(fql_gemm16_euler_kernel<false>), PLAN_K_GEMM16_EULER, 0, 0}, {plan_fn(fql_gemm16_euler_kernel<true>), PLAN_K_GEMM16_EULER_KBIG, 0, 0},
        {plan_fn(fql_side_kernel), PLAN_K_SIDE, 0, 0}, {plan_fn(fql_side_split_kernel), PLAN_K_SIDE_SPLIT, 0, 0},
        {plan_fn(fql_side_big_kernel), PLAN_K_SIDE_BIG, 0, 0}, FQL_PLAN_CHAIN(256), FQL_PLAN_CHAIN(512),
        // the same launches with their tasks in the kernel arguments: the entry names the tile bodies, fql_debug_task_forms the form
        {plan_fn(fql_side_ka_kernel), PLAN_K_SIDE, 0, 0}, {plan_fn(fql_side_split_ka_kernel), PLAN_K_SIDE_SPLIT, 0, 0},
        {plan_fn(fql_side_big_ka_kernel), PLAN_K_SIDE_BIG, 0, 0}};
#undef FQL_PLAN_CHAIN
    return t;
}
}  // namespace
extern "C" int fql_debug_plan(fql_handle h, void* out, size_t bytes) {
    if (!h || (bytes && !out) || bytes % sizeof(int32_t)) return FQL_E_INVALID;
    if (h->visual || !h->prog_full.exec || h->prog_full.launches.empty()) return FQL_E_STATE;
    try {
        const Program& pr = h->prog_full;
        std::vector<int32_t> plan{0, (int32_t)pr.launches.size()};
        for (size_t i = 0; i < pr.launches.size(); ++i) {
            const Launch& L = pr.launches[i];
            const Bound& d = L.k;
            PlanKernel k{d.fn, PLAN_K_OTHER, 0, 0};
            for (const PlanKernel& c : plan_kernels()) if (c.fn == d.fn) k = c;
            const bool table = L.type == OP_GEMM || L.type == OP_GEMM64;   // (other launches keep no task table)
            const bool chain = L.type == OP_CHAIN;
            if (chain != (k.entry == PLAN_K_CHAIN || k.entry == PLAN_K_CHAIN_SPLIT)) throw HipError{"internal: a chain launch binds an unknown kernel"};
            if (table == (k.entry == PLAN_K_OTHER || chain)) throw HipError{"internal: a GEMM launch binds an unknown kernel"};
            plan.insert(plan.end(), {(int32_t)i, L.lane, (int32_t)L.type, (int32_t)d.workgroups(), k.entry,
                                     table ? (int32_t)L.h_gemm.size() : 0, table ? (int32_t)L.h_wgrad.size() : 0, table ? (int32_t)L.h_ln.size() : 0,
                                     chain ? 1 : 0});
            if (table) {
                for (const GemmTask& t : L.h_gemm) plan.insert(plan.end(), {t.M, t.N, t.K, (L.type == OP_GEMM ? 16 : 32) * t.tmt, t.wk, t.xg});
                for (const WgradTask& t : L.h_wgrad) plan.insert(plan.end(), {t.M, t.Kin, t.N, k.entry == PLAN_K_SIDE_SPLIT ? 1 : 0});
                for (const LnBwdTask& t : L.h_ln) plan.push_back(t.M);
            }
            if (chain) {
                ChainArgs ca;
                if (d.args.size() < sizeof(ChainArgs)) throw HipError{"internal: a chain launch binds no ChainArgs"};
                std::memcpy(&ca, d.args.data(), sizeof(ChainArgs));
                plan.insert(plan.end(), {ca.M, k.H, k.V, ca.xg, k.entry == PLAN_K_CHAIN_SPLIT ? 1 : 0});
            }
        }
        plan[0] = (int32_t)plan.size();
        if (bytes > plan.size() * sizeof(int32_t)) return FQL_E_INVALID;
        if (bytes) std::memcpy(out, plan.data(), bytes);
        return FQL_OK;
    } catch (...) {
        return FQL_E_HIP;
    }
}

int fql_dataset_upload_frames(fql_handle h, int64_t n, const uint8_t* frames, const uint8_t* next_frames, const float* act,
                              const float* rew, const float* mask, const float* terminals, int frame_stack, float p_aug) {
    FQL_ADMIT(h, EP_dataset_upload_frames);
    if (!h) return FQL_E_INVALID;
    FQL_TRY(h, {
        if (!h->visual) throw Invalid{"fql_dataset_upload_frames needs an agent created with an encoder"};
        if (n <= 0 || !frames || !next_frames || !act || !rew || !mask || !terminals) invalid("frames dataset pointers must not be NULL (n=%lld)", (long long)n);
        if (frame_stack < 1 || h->cfg.img_c % frame_stack) invalid("frame_stack %d must divide the %d image channels", frame_stack, h->cfg.img_c);
        if (p_aug < 0.f || p_aug > 1.f) invalid("p_aug must be in [0, 1]");
        HIP_CHECK(hipDeviceSynchronize());
        hipFree(h->ds_frames); hipFree(h->ds_next_frames); hipFree(h->ds_init);
        hipFree(h->ds_act); hipFree(h->ds_rew); hipFree(h->ds_mask);
        h->ds_frames = h->ds_next_frames = nullptr; h->ds_init = nullptr; h->ds_act = h->ds_rew = h->ds_mask = nullptr;
        const size_t fb = (size_t)h->cfg.img_h * h->cfg.img_w * (h->cfg.img_c / frame_stack);
        HIP_CHECK(hipMalloc((void**)&h->ds_frames, (size_t)n * fb));
        HIP_CHECK(hipMalloc((void**)&h->ds_next_frames, (size_t)n * fb));
        HIP_CHECK(hipMemcpy(h->ds_frames, frames, (size_t)n * fb, hipMemcpyDefault));
        HIP_CHECK(hipMemcpy(h->ds_next_frames, next_frames, (size_t)n * fb, hipMemcpyDefault));
        auto up = [&](float*& dst, const float* src, size_t w) {
            HIP_CHECK(hipMalloc((void**)&dst, (size_t)n * w * sizeof(float)));
            HIP_CHECK(hipMemcpy(dst, src, (size_t)n * w * sizeof(float), hipMemcpyDefault));
        };
        up(h->ds_act, act, h->cfg.act_dim); up(h->ds_rew, rew, 1); up(h->ds_mask, mask, 1);
        // utils/datasets.py:58-62: terminal_locs = nonzero(terminals > 0); initial_locs = [0, terminal_locs[:-1] + 1];
        // a row's episode start = the last initial_loc <= row (searchsorted(..., side='right') - 1, utils/datasets.py:75)
        std::vector<float> term((size_t)n);
        HIP_CHECK(hipMemcpy(term.data(), terminals, (size_t)n * sizeof(float), hipMemcpyDefault));
        std::vector<int64_t> tl;
        for (int64_t i = 0; i < n; ++i) if (term[i] > 0.f) tl.push_back(i);
        std::vector<int64_t> init((size_t)n);
        int64_t cur = 0;
        size_t k = 0;   // next terminal whose successor may start an episode; the LAST terminal never starts one (terminal_locs[:-1])
        for (int64_t i = 0; i < n; ++i) {
            while (k + 1 < tl.size() && tl[k] + 1 <= i) { cur = tl[k] + 1; ++k; }
            init[i] = cur;
        }
        HIP_CHECK(hipMalloc((void**)&h->ds_init, (size_t)n * sizeof(int64_t)));
        HIP_CHECK(hipMemcpy(h->ds_init, init.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        h->ds_fs = frame_stack; h->ds_paug = p_aug;
        h->ds_size = n; h->ds_cap = n; h->ds_ptr = 0;
        h->src_valid = false;
    });
}
int fql_update_from_frames(fql_handle h, const int64_t* idx, const int32_t* crop_froms, int batch_size, int64_t lo, int64_t hi,
                           const fql_noise* noise, float* info13, void* stream) {
    FQL_ADMIT(h, EP_update_from_frames);
    if (!h) return FQL_E_INVALID;
    return update_with(h, h->prog_full, info13, FQL_NUM_INFO, stream, [&](hipStream_t s) {
        h->hip_touch();
        h->source_from_frames(idx, crop_froms, batch_size, lo, hi, noise, s);
    });
}

#include "fql_engine_groups.h"

// Part of fql_engine.hip, not a unit of its own: agent groups and their entry points.  Needs everything else of fql_engine.hip.
// ================================================================================================
// Agent groups: K members of one structure advanced by ONE fused update program.
// The members' prog_full are zipped launch by launch.  A table-driven launch becomes one launch over the concatenation of the members'
// task tables (tile0 and the side kernel's sub-table offsets rebased, grid = the sum); an argument-struct launch becomes one launch of the
// kernel's multi-instance entry point with blockIdx.y = member, reading the member's argument struct from a device array.  Every task keeps
// the tile shape and arguments its member's program gave it, so each member computes exactly what it computes alone.
// The members' sampling programs are zipped the same way (fql_group_s::Sample): one fused sampling call for all K.
// A group has a kind, its members': what a kind's group fuses, what may differ between its members and how it samples is the kind's row
// of k_group_kinds, below.  A new group kind adds its row, the multi-instance entries of its kernels and its C entry points.
// ================================================================================================
namespace {

typedef Bound (*MultiBind)(Geo g, const void* args);   // the multi-instance kernel bound over a device array of argument structs
struct MultiEntry {
    MultiBind bind;
    size_t arg_bytes;   // what the single-instance launch binds (Bound::args)
    size_t stride;      // the element of the multi-instance kernel's array: those bytes, padded to the struct's size
};
// single-instance kernel -> its multi-instance entry point
const std::map<const void*, MultiEntry>& multi_entries() {
    static const std::map<const void*, MultiEntry> m = [] {
        std::map<const void*, MultiEntry> e;
#define FQL_MULTI(single, multi, A) \
    e[(const void*)(single)] = MultiEntry{[](Geo g, const void* a) { return bind(multi, g, (const A*)a); }, sizeof(A), sizeof(A)}
        FQL_MULTI(fql_prep_kernel, fql_prep_multi_kernel, PrepArgs);
        FQL_MULTI(fql_loss_actor_kernel, fql_loss_actor_multi_kernel, LossActorArgs);
        FQL_MULTI(fql_euler_finish_kernel, fql_euler_finish_multi_kernel, EulerFinishArgs);
        FQL_MULTI(fql_head_dgrad_kernel, fql_head_dgrad_multi_kernel, GemmTask);
        FQL_MULTI(fql_dgrad0_kernel, fql_dgrad0_multi_kernel, Dgrad0Args);
        FQL_MULTI(fql_adam_kernel, fql_adam_multi_kernel, AdamArgs);
        FQL_MULTI(fql_finalize_kernel, fql_finalize_multi_kernel, FinalizeArgs);
        FQL_MULTI((fql_chain_kernel<512, 0>), (fql_chain_multi_kernel<512, 0>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<512, 1>), (fql_chain_multi_kernel<512, 1>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<512, 2>), (fql_chain_multi_kernel<512, 2>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<512, 3>), (fql_chain_multi_kernel<512, 3>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<256, 0>), (fql_chain_multi_kernel<256, 0>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<256, 1>), (fql_chain_multi_kernel<256, 1>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<256, 2>), (fql_chain_multi_kernel<256, 2>), ChainArgs);
        FQL_MULTI((fql_chain_kernel<256, 3>), (fql_chain_multi_kernel<256, 3>), ChainArgs);
        // ReBRAC (fql_rebrac.h)
        FQL_MULTI(fql_rebrac_prep_kernel, fql_rebrac_prep_multi_kernel, RebracPrepArgs);
        FQL_MULTI(fql_rebrac_act_kernel, fql_rebrac_act_multi_kernel, RebracActArgs);
        FQL_MULTI(fql_rebrac_loss_critic_kernel, fql_rebrac_loss_critic_multi_kernel, RebracCriticArgs);
        FQL_MULTI(fql_rebrac_loss_actor_kernel, fql_rebrac_loss_actor_multi_kernel, RebracActorArgs);
        FQL_MULTI(fql_rebrac_actor_grad_kernel, fql_rebrac_actor_grad_multi_kernel, RebracActorGradArgs);
        // (FinalizeArgs, int full): the launch binds the two arguments packed, the array element is the struct that holds both
        FQL_MULTI(fql_rebrac_finalize_kernel, fql_rebrac_finalize_multi_kernel, RebracFinalizeArgs);
        e[(const void*)fql_rebrac_finalize_kernel].arg_bytes = packed_bytes<FinalizeArgs, int>();
        // IQL-diffusion (fql_iqld.h; its value loss is IFQL's, its sampler's row assembly BC's): the update programs, then the sweep sampler
        FQL_MULTI(fql_iqld_prep_kernel, fql_iqld_prep_multi_kernel, IqldPrepArgs);
        FQL_MULTI(fql_ifql_loss_value_kernel, fql_ifql_loss_value_multi_kernel, IfqlValueArgs);
        FQL_MULTI(fql_iqld_loss_critic_kernel, fql_iqld_loss_critic_multi_kernel, IqldCriticArgs);
        FQL_MULTI(fql_iqld_weight_kernel, fql_iqld_weight_multi_kernel, IqldWeightArgs);
        FQL_MULTI(fql_iqld_loss_actor_kernel, fql_iqld_loss_actor_multi_kernel, IqldActorLossArgs);
        FQL_MULTI(fql_iqld_embed_grad_kernel, fql_iqld_embed_grad_multi_kernel, IqldEmbedGradArgs);   // grid (2, members)
        FQL_MULTI(fql_iqld_finalize_kernel, fql_iqld_finalize_multi_kernel, IqldFinalizeArgs);
        FQL_MULTI(fql_bc_assemble_kernel, fql_bc_assemble_multi_kernel, BcAssembleArgs);
        FQL_MULTI(fql_iqld_stepbias_kernel, fql_iqld_stepbias_multi_kernel, IqldStepBiasArgs);
        FQL_MULTI(fql_iqld_layer0_kernel, fql_iqld_layer0_multi_kernel, IqldLayer0Args);
        FQL_MULTI(fql_iqld_cfg_layer0_kernel, fql_iqld_cfg_layer0_multi_kernel, IqldCfgLayer0Args);
        FQL_MULTI(fql_iqld_cfg_rows_step_kernel, fql_iqld_cfg_rows_step_multi_kernel, IqldCfgRowsStepArgs);
        // IFQL (fql_ifql.h): the update program (its value loss is entered above; the sampler's three kernels are bound by sample_ws_bon)
        FQL_MULTI(fql_ifql_prep_kernel, fql_ifql_prep_multi_kernel, IfqlPrepArgs);
        FQL_MULTI(fql_ifql_loss_critic_kernel, fql_ifql_loss_critic_multi_kernel, IfqlCriticArgs);
        FQL_MULTI(fql_ifql_finalize_kernel, fql_ifql_finalize_multi_kernel, FinalizeArgs);
        // IQL (fql_iql.h; its value and critic losses are IFQL's, entered above; the sampler's head is bound by sample_ws)
        FQL_MULTI(fql_iql_prep_kernel, fql_iql_prep_multi_kernel, IqlPrepArgs);
        FQL_MULTI(fql_iql_head_kernel, fql_iql_head_multi_kernel, IqlHeadArgs);
        FQL_MULTI(fql_iql_loss_awr_kernel, fql_iql_loss_awr_multi_kernel, IqlAwrArgs);
        FQL_MULTI(fql_iql_loss_ddpgbc_kernel, fql_iql_loss_ddpgbc_multi_kernel, IqlDdpgArgs);
        FQL_MULTI(fql_iql_actor_grad_kernel, fql_iql_actor_grad_multi_kernel, IqlActorGradArgs);
        FQL_MULTI(fql_iql_finalize_kernel, fql_iql_finalize_multi_kernel, IqlFinalizeArgs);
        // CFGRL (fql_cfgrl.h): the update program, then the sweep sampler, which ends on IQL-diffusion's rows step kernel, entered above
        // (the sampler's row assembly is bound by sample_ws_cfg)
        FQL_MULTI(fql_cfgrl_prep_kernel, fql_cfgrl_prep_multi_kernel, CfgrlPrepArgs);
        FQL_MULTI(fql_cfgrl_embed_grad_kernel, fql_cfgrl_embed_grad_multi_kernel, CfgrlEmbedGradArgs);   // grid (1, members)
        FQL_MULTI(fql_cfgrl_finalize_kernel, fql_cfgrl_finalize_multi_kernel, FinalizeArgs);
        FQL_MULTI(fql_cfgrl_assemble_kernel, fql_cfgrl_assemble_multi_kernel, CfgrlAssembleArgs);
        FQL_MULTI(fql_cfgrl_layer0_kernel, fql_cfgrl_layer0_multi_kernel, CfgrlLayer0Args);
        FQL_MULTI(fql_cfgrl_cfg_layer0_kernel, fql_cfgrl_cfg_layer0_multi_kernel, CfgrlCfgLayer0Args);
        // SAC (fql_sac.h): the update program; the sampler's last launch is the act kernel's multi-instance entry, bound by sample_ws
        FQL_MULTI(fql_sac_prep_kernel, fql_sac_prep_multi_kernel, SacPrepArgs);
        FQL_MULTI(fql_sac_act_kernel, fql_sac_act_multi_kernel, SacActArgs);
        FQL_MULTI(fql_sac_loss_critic_kernel, fql_sac_loss_critic_multi_kernel, SacCriticArgs);
        FQL_MULTI(fql_sac_loss_actor_kernel, fql_sac_loss_actor_multi_kernel, SacActorArgs);
        FQL_MULTI(fql_sac_actor_grad_kernel, fql_sac_actor_grad_multi_kernel, SacActorGradArgs);
        FQL_MULTI(fql_sac_finalize_kernel, fql_sac_finalize_multi_kernel, FinalizeArgs);
#undef FQL_MULTI
        return e;
    }();
    return m;
}

bool is_table_launch(OpType t) { return t == OP_GEMM || t == OP_GEMM64 || t == OP_WFRAG; }

struct GLaunch {
    int lane = 0;
    std::vector<int> waits;
    bool record_after = false;
    hipEvent_t ev = nullptr;
    int form = 0;   // fql_debug_task_forms' word
    // table-driven: the launch over the members' concatenated tables, bound like a member's own; argument-struct: the kernel's
    // multi-instance entry point, grid y = member, over the [K] argument structs in device memory
    Bound k;
};
// one fused update program: the zip of one program of every member, captured as one graph (what issue_lanes needs of a launch list)
struct GProgram {
    std::vector<GLaunch> launches;
    bool lane_used[FQL_LANES] = {};
    hipEvent_t ev_fork = nullptr, ev_join[FQL_LANES] = {};
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// ---- one row per group kind ----
// What may differ between the members of a group beside the create seed are kernel ARGUMENTS; everything else is structure, or a constant
// every member shares.  same_structure: the members' configs with those free fields (and the batch size, which the members' B answers)
// zeroed, compared byte by byte.
template <typename C, typename Zero>
bool same_but(C a, C b, Zero zero) { zero(a); zero(b); return std::memcmp(&a, &b, sizeof a) == 0; }
bool same_base(const fql_engine& a, const fql_engine& b) { return same_but(a.cfg, b.cfg, [](fql_config& c) { c.batch_size = 0; }); }
bool same_fql(const fql_engine& a, const fql_engine& b) { return same_but(a.cfg, b.cfg, [](fql_config& c) { c.alpha = 0.f; c.batch_size = 0; }); }
bool same_rebrac(const fql_engine& a, const fql_engine& b) {
    return same_base(a, b) && same_but(a.rcfg, b.rcfg, [](fql_rebrac_config& c) { c.alpha_actor = c.alpha_critic = 0.f; });
}
// (both reach the device as IqldWeightArgs::temp alone)
bool same_iqld(const fql_engine& a, const fql_engine& b) {
    return same_base(a, b) && same_but(a.dcfg, b.dcfg, [](fql_iqld_config& c) { c.awr_temperature = c.softmax_beta = 0.f; });
}
// (IfqlValueArgs::expectile alone; num_samples is structure: it sets the row count of the sampler's workspaces)
bool same_ifql(const fql_engine& a, const fql_engine& b) { return same_base(a, b) && a.num_samples == b.num_samples; }
// (IfqlValueArgs::expectile; IqlAwrArgs / IqlDdpgArgs / IqlActorGradArgs::alpha; actor_loss and const_std are structure: they choose the
// launches and the log_stds leaf)
bool same_iql(const fql_engine& a, const fql_engine& b) {
    return same_base(a, b) && same_but(a.qcfg, b.qcfg, [](fql_iql_config& c) { c.expectile = c.alpha = 0.f; });
}
// (cfg is the sampler's default guidance weight, an argument of the sampling calls; the three goal-mixture probabilities reach the
// device only as CfgrlSrc::thr_traj, p_cur and all_cur, which every update writes per member; goal_dim, flow_steps and p_uncond are
// structure or shared constants)
bool same_cfgrl(const fql_engine& a, const fql_engine& b) {
    return same_base(a, b) && same_but(a.gcfg, b.gcfg, [](fql_cfgrl_config& c) {
               c.cfg = 0.f;
               c.actor_p_curgoal = c.actor_p_trajgoal = c.actor_p_randomgoal = 0;
           });
}
// (target_entropy - NaN = automatic - and the multiplier it is then derived from reach the device as SacActorArgs::target_entropy alone;
// tanh_squash, backup_entropy, q_agg and the rest choose kernel arguments every member shares)
bool same_sac(const fql_engine& a, const fql_engine& b) {
    return same_base(a, b) && same_but(a.scfg, b.scfg, [](fql_sac_config& c) { c.target_entropy = c.target_entropy_multiplier = 0.f; });
}

// The launch that ends a chunk of the plain chunk loop (fql_group_s::sample), over the [K] argument structs behind the chunk's [K]
// AssembleArgs.  bind: the multi-instance kernel over `n_pad` padded rows per member (a chunk's m <= n_pad: what lies past m returns at
// once); fill: member i's struct of a chunk of `mm` rows from row `start`, every argument as the member's own call fills it
// (fql_engine::eval_rows, fql_engine::sample_actor): its noise rows z or null, where its actions go, its seed.
struct ChunkRows { const float* z; float* dst; uint64_t seed; int mm, start; float temperature; };
struct SampleFinish {
    Bound (*bind)(int n_pad, int ad, int K, const void* d);
    void (*fill)(void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, bool flow, const ChunkRows& r);
    size_t bytes;
};
Geo per_element(int n, int threads, int K) { return Geo(dim3((n + threads - 1) / threads, K), dim3(threads), 0); }
const SampleFinish k_finish_extract = {
    [](int n_pad, int ad, int K, const void* d) { return bind(fql_extract_multi_kernel, per_element(n_pad * ad, 256, K), (const ExtractArgs*)d); },
    [](void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, bool flow, const ChunkRows& r) {
        ((ExtractArgs*)a)[i] = ExtractArgs{flow ? ev.tgt : ev.p_os.out, r.dst, r.mm, e.cfg.act_dim, pad16(e.cfg.act_dim)};
    },
    sizeof(ExtractArgs)};
// ReBRAC: fql_rebrac_act_multi_kernel on the actor's forward writes the actions where extract-multi would
const SampleFinish k_finish_rebrac = {
    [](int n_pad, int ad, int K, const void* d) { return bind(fql_rebrac_act_multi_kernel, per_element(n_pad * ad, FQL_THREADS, K), (const RebracActArgs*)d); },
    [](void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, bool, const ChunkRows& r) {
        const int ad = e.cfg.act_dim;
        ((RebracActArgs*)a)[i] = RebracActArgs{ev.p_os.out, r.z, r.dst, e.seed, r.seed, r.mm, ad, pad16(ad), ad, ad, 0, r.start, r.z ? 1 : 2, e.rcfg.tanh_squash, 1,
                                               e.rcfg.actor_noise * r.temperature, e.rcfg.actor_noise_clip};
    },
    sizeof(RebracActArgs)};
// IQL: fql_iql_sample_multi_kernel on the means - each member's own row numbers (row0 = start), seed, key and log_stds (P + ls_off, null
// under const_std), one temperature
const SampleFinish k_finish_iql = {
    [](int n_pad, int ad, int K, const void* d) { return bind(fql_iql_sample_multi_kernel, per_element(n_pad * ad, FQL_THREADS, K), (const IqlSampleArgs*)d); },
    [](void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, bool, const ChunkRows& r) {
        const int ad = e.cfg.act_dim;
        ((IqlSampleArgs*)a)[i] = IqlSampleArgs{ev.p_os.out, e.qcfg.const_std ? nullptr : e.P + e.ls_off, r.z, r.dst, e.seed, r.seed, r.mm, ad, pad16(ad), r.start, r.temperature};
    },
    sizeof(IqlSampleArgs)};
// SAC: fql_sac_act_multi_kernel, one thread per row, on the actor's forward, whose last layer is the [H, 2 ap] head layer - noise_mode 1
// or 2, clip_out 1, no lp
const SampleFinish k_finish_sac = {
    [](int n_pad, int, int K, const void* d) { return bind(fql_sac_act_multi_kernel, per_element(n_pad, FQL_THREADS, K), (const SacActArgs*)d); },
    [](void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, bool, const ChunkRows& r) {
        const int ad = e.cfg.act_dim;
        ((SacActArgs*)a)[i] = SacActArgs{ev.p_os.out, r.z, r.dst, r.dst, nullptr, e.seed, r.seed, r.mm, ad, pad16(ad), ad, ad, 0, r.start, r.mm, r.z ? 1 : 2, e.scfg.tanh_squash, 1,
                                         r.temperature};
    },
    sizeof(SacActArgs)};

// The row assembly that opens a chunk of the guidance-sweep loop (fql_group_s::sample_cfg), over the chunk's [K] argument structs; its
// [K] ExtractArgs lie behind them.  goals: member i's goal rows of the chunk, where the kind has them.
struct SweepAssemble {
    Bound (*bind)(int half, int K, const void* d);
    void (*fill)(void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, const float* obs, const float* goals, int half, const ChunkRows& r);
    size_t bytes;
};
const SweepAssemble k_assemble_bc = {
    [](int half, int K, const void* d) { return bind(fql_bc_assemble_multi_kernel, Geo(dim3((half + 3) / 4, K), dim3(FQL_THREADS), 0), (const BcAssembleArgs*)d); },
    [](void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, const float* obs, const float*, int half, const ChunkRows& r) {
        const int ad = e.cfg.act_dim;
        ((BcAssembleArgs*)a)[i] = BcAssembleArgs{obs, r.z, ev.X, ev.Xf, e.seed, r.seed, r.mm, half, e.cfg.obs_dim, ad, e.nets[NET_BC].in_p(), pad16(ad), r.start};
    },
    sizeof(BcAssembleArgs)};
// CFGRL's writes both halves - [obs | goal] and [obs | the member's own unc_embed leaf]
const SweepAssemble k_assemble_cfgrl = {
    [](int half, int K, const void* d) { return bind(fql_cfgrl_assemble_multi_kernel, Geo(dim3((half + 3) / 4, K), dim3(FQL_THREADS), 0), (const CfgrlAssembleArgs*)d); },
    [](void* a, int i, const fql_engine& e, const fql_engine::Eval& ev, const float* obs, const float* goals, int half, const ChunkRows& r) {
        const int ad = e.cfg.act_dim;
        ((CfgrlAssembleArgs*)a)[i] = CfgrlAssembleArgs{obs, goals, e.P + e.emb_off, r.z, ev.X, ev.Xf, e.seed, r.seed, r.mm, half, e.cfg.obs_dim, e.gcfg.goal_dim, ad,
                                                       e.nets[NET_BC].in_p(), pad16(ad), r.start};
    },
    sizeof(CfgrlAssembleArgs)};

// What a group call does; GroupKind::calls names the call of each kind of group that does it, as the refusal on a group of that kind
// says it: "<fn> is not available on a group of <kind> agents (<hint>)"
enum GroupCall { GC_UPDATE, GC_SAMPLE, GC_STATS, GC_FLOW };
enum GroupSampler { GS_PLAIN, GS_SWEEP, GS_BEST_OF_N };
struct GroupKind {
    AgentKind kind;        // the row's index
    const char* create;    // its create call; nullptr: the kind has no groups
    const char* takes;     // what that call's refusal of another kind's member says
    const char* grouped_by;   // what the other creates' refusal of a member of THIS kind adds, or nullptr
    const char* free_fields;  // what may differ between members beside the create seed ...
    bool (*same_structure)(const fql_engine&, const fql_engine&);   // ... and the compare that lets exactly that differ
    int programs;          // fused update programs (fql_group_s::progs): prog_full; + prog_critic; + prog_actor, prog_none
    int infos;             // floats per member of an update's infos where that is not the members' num_info(), else 0
    bool goals;            // every update sets each member's goal source (CfgrlSrc) beside its dataset source, and the sampler takes goals
    const char* calls[4];  // by GroupCall
    GroupSampler sampler;  // the chunk loop of its sample_actions
    const SampleFinish* finish;      // GS_PLAIN, and GS_BEST_OF_N's flow call: assemble-multi, the members' program, this launch
    const SweepAssemble* assemble;   // GS_SWEEP: this launch, the members' sweep program, extract-multi
};
constexpr GroupKind k_group_kinds[kNumKinds] = {
    {AgentKind::FQL, "fql_group_create", "groups take FQL agents only", nullptr, "alpha", same_fql, 1, 0, false,
     {"fql_group_update_from_dataset", "fql_group_sample_actions", "fql_group_sample_stats", "fql_group_flow_actions"}, GS_PLAIN, &k_finish_extract, nullptr},
    // the one fused program; sample_actions zips the members' Euler flow and critic pair between the multi-instance
    // forms of IFQL's three sampling kernels (fql_group_s::sample_bon); the members have no one-step actor
    {AgentKind::IFQL, "fql_ifql_group_create", "IFQL groups take IFQL agents only", nullptr, "expectile", same_ifql, 1, 0, false,
     {"fql_ifql_group_update_from_dataset", "best of num_samples: fql_ifql_group_sample_actions", "fql_ifql_group_stats", "fql_ifql_group_flow_actions"},
     GS_BEST_OF_N, &k_finish_extract, nullptr},
    // a second fused program, the zip of the members' critic-only step; infos in fql_rebrac_update's layout, the
    // 13 floats of DevState::info per member (12 or 7 by the step's kind, zeros behind them)
    {AgentKind::REBRAC, "fql_rebrac_group_create", "ReBRAC groups take ReBRAC agents only", nullptr, "alpha_actor / alpha_critic", same_rebrac, 2, FQL_NUM_INFO, false,
     {"the step kind is an argument: fql_rebrac_group_update_from_dataset", "fql_rebrac_group_sample_actions", "fql_rebrac_group_stats",
      "the actor is deterministic: fql_rebrac_group_sample_actions"},
     GS_PLAIN, &k_finish_rebrac, nullptr},
    // the one fused program, entered with each member's dataset source or with its two-source balanced one (the
    // member's own replay ring)
    {AgentKind::SAC, "fql_sac_group_create", "SAC groups take SAC agents only", nullptr, "target_entropy / target_entropy_multiplier", same_sac, 1, 0, false,
     {"fql_sac_group_update_from_dataset (or fql_sac_group_update_balanced)", "it takes a temperature: fql_sac_group_sample_actions", "fql_sac_group_stats",
      "the actor is a Gaussian, there is no flow: fql_sac_group_sample_actions"},
     GS_PLAIN, &k_finish_sac, nullptr},
    {AgentKind::BC, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, false, {}, GS_PLAIN, nullptr, nullptr},
    // the one fused program - IFQL's value and critic lanes beside the Gaussian actor's own kernels
    {AgentKind::IQL, "fql_iql_group_create", "IQL groups take IQL agents only", nullptr, "expectile / alpha", same_iql, 1, 0, false,
     {"fql_iql_group_update_from_dataset", "it takes a temperature: fql_iql_group_sample_actions", "fql_iql_group_stats",
      "the actor is a Gaussian, there is no flow: fql_iql_group_sample_actions"},
     GS_PLAIN, &k_finish_iql, nullptr},
    // one fused program per step kind (full, critic-only, actor-only, neither); the sampler zips the members' sweep
    // program: one guidance weight per row
    {AgentKind::IQLD, "fql_iqld_group_create", "IQL-diffusion groups take IQL-diffusion agents only", nullptr, "awr_temperature / softmax_beta", same_iqld, 4, 0, false,
     {"the step kind is two arguments: fql_iqld_group_update_from_dataset", "it takes guidance weights: fql_iqld_group_sample_actions", "fql_iqld_group_stats",
      "it takes guidance weights: fql_iqld_group_sample_actions"},
     GS_SWEEP, nullptr, &k_assemble_bc},
    // the one fused program - BC's single lane; the sampler zips the members' sweep program behind CFGRL's two-half
    // row assembly
    {AgentKind::CFGRL, "fql_cfgrl_group_create", "CFGRL groups take CFGRL agents only", "; CFGRL agents are grouped by fql_cfgrl_group_create",
     "cfg / actor_p_curgoal / actor_p_trajgoal / actor_p_randomgoal", same_cfgrl, 1, 0, true,
     {"it sets each member's goal source: fql_cfgrl_group_update_from_dataset", "it takes goals and guidance weights: fql_cfgrl_group_sample_actions",
      "fql_cfgrl_group_stats", "it takes goals and guidance weights: fql_cfgrl_group_sample_actions"},
     GS_SWEEP, nullptr, &k_assemble_cfgrl},
};
constexpr bool group_rows_in_order() {
    for (int i = 0; i < kNumKinds; ++i) if ((int)k_group_kinds[i].kind != i) return false;
    return true;
}
static_assert(group_rows_in_order(), "k_group_kinds is indexed by AgentKind");
// the update programs a group fuses, in the order of fql_group_s::progs: the first GroupKind::programs of these
constexpr Program fql_engine::* k_group_programs[] = {&fql_engine::prog_full, &fql_engine::prog_critic, &fql_engine::prog_actor, &fql_engine::prog_none};

}  // namespace

struct fql_group_s {
    std::vector<fql_handle> m;
    const GroupKind* kind = nullptr;     // the members' kind: its row of k_group_kinds
    int K = 0, B = 0;
    hipStream_t lanes[FQL_LANES] = {};   // lane 0 = the group's own stream
    // One fused program per entry of k_group_programs, the first kind->programs of them: the members' prog_full zipped, their
    // prog_critic, their prog_actor and prog_none
    enum { FULL = 0, CRITIC = 1, ACTOR = 2, NONE = 3, MAX_PROGS = 4 };
    GProgram progs[MAX_PROGS];
    hipEvent_t ev_in = nullptr, ev_done = nullptr;
    std::vector<void*> allocs;
    int64_t* d_idx = nullptr;   // [K][B] staging of host row indices
    unsigned char* d_mask = nullptr;   // a CFGRL group: [K][B] staging of a host do_cfg mask
    hipStream_t last = nullptr; // the stream of the last group call (update or sampling): a call on another stream waits for that one first

    void* galloc(size_t bytes) {
        void* d = nullptr;
        HIP_CHECK(hipMalloc(&d, std::max<size_t>(bytes, 16)));
        allocs.push_back(d);
        return d;
    }
    void* upload(const void* src, size_t bytes) {
        void* d = galloc(bytes);
        if (bytes) HIP_CHECK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        return d;
    }
    // the members' task tables (their host copies) one after the other into `all` and onto the device, each member's tile0 shifted by
    // `shift[member]` (MiscTask: no tile0, no shift)
    template <typename T>
    void* fuse(const std::vector<const std::vector<T>*>& tables, const std::vector<int>& shift, std::vector<T>& all) {
        all.clear();
        for (size_t i = 0; i < tables.size(); ++i)
            for (T t : *tables[i]) { rebase_tile0(t, shift[i]); all.push_back(t); }
        return upload(all.data(), all.size() * sizeof(T));
    }
    template <typename T> static void rebase_tile0(T& t, int d) { t.tile0 += d; }
    static void rebase_tile0(MiscTask&, int) {}   // (indexed by workgroup - tile_m: concatenation is the rebase)

    // one fused launch from launch `li` of every member's program `prog(member)`: the update's prog_full, or a sampling workspace's
    template <typename Sel>
    GLaunch zip(int li, Sel&& prog) {
        const Launch& L0 = prog(*m[0]).launches[li];
        GLaunch G;
        G.lane = L0.lane; G.waits = L0.waits; G.record_after = L0.record_after;
        if (is_table_launch(L0.type)) {
            Launch F;   // bound by the family's helper of schedule(): the fused launch takes the form ITS task counts allow
            F.type = L0.type;
            std::vector<const std::vector<GemmTask>*> tg;
            std::vector<const std::vector<WgradTask>*> tw;
            std::vector<const std::vector<LnBwdTask>*> tl;
            std::vector<const std::vector<MiscTask>*> tm;
            std::vector<const std::vector<WfragTask>*> tf;
            std::vector<int> sg, sw, sl, sm;
            int cg = 0, cw = 0, cl = 0, cm = 0;
            for (int k = 0; k < K; ++k) {
                const Launch& L = prog(*m[k]).launches[li];
                sg.push_back(cg); sw.push_back(cw); sl.push_back(cl); sm.push_back(0);
                if (L0.type == OP_WFRAG) { tf.push_back(&m[k]->h_wfrag); cg += m[k]->wfrag_grid; }
                else if (L0.type == OP_GEMM64) {
                    tg.push_back(&L.h_gemm); cg += L.tile_w;
                    tw.push_back(&L.h_wgrad); cw += L.tile_l - L.tile_w;
                    tl.push_back(&L.h_ln); cl += L.tile_m - L.tile_l;
                    tm.push_back(&L.h_misc); cm += L.grid - L.tile_m;
                } else { tg.push_back(&L.h_gemm); cg += L.grid; }
            }
            if (L0.type == OP_WFRAG) {
                std::vector<WfragTask> h_wf;
                F.table = fuse(tf, sg, h_wf); F.ntasks = (int)h_wf.size(); F.grid = cg;
                F.k = bind(fql_wfrag_kernel, F.grid, (const WfragTask*)F.table, F.ntasks, -1);
            } else if (L0.type == OP_GEMM64) {
                F.table = fuse(tg, sg, F.h_gemm);
                F.table_w = fuse(tw, sw, F.h_wgrad);
                F.table_l = fuse(tl, sl, F.h_ln);
                F.table_m = fuse(tm, sm, F.h_misc);
                F.ntasks = (int)F.h_gemm.size(); F.n_w = (int)F.h_wgrad.size(); F.n_l = (int)F.h_ln.size();
                F.tile_w = cg; F.tile_l = cg + cw; F.tile_m = cg + cw + cl; F.grid = F.tile_m + cm;
                m[0]->bind_side(F, L0.k.lds);
            } else {
                F.table = fuse(tg, sg, F.h_gemm);
                F.ntasks = (int)F.h_gemm.size(); F.grid = cg;
                m[0]->bind_gemm16(F);
            }
            G.k = F.k;
            G.form = F.ka ? 2 : 1;
            return G;
        }
        const Bound& k0 = L0.k;
        auto it = multi_entries().find(k0.fn);
        if (it == multi_entries().end()) invalid("agent groups: launch %d (op type %d) has no multi-instance kernel", li, (int)L0.type);
        std::vector<uint8_t> args;
        for (int k = 0; k < K; ++k) {   // the structs are exactly what the member's own issue() passes
            const Launch& L = prog(*m[k]).launches[li];
            if (L.k.args.size() != it->second.arg_bytes) invalid("internal: launch %d binds %zu argument bytes, its struct has %zu", li, L.k.args.size(), it->second.arg_bytes);
            alignas(16) unsigned char a[FQL_BOUND_BYTES];
            m[k]->issue_args(L, m[k]->tl_of(prog(*m[k]), L), a);
            args.insert(args.end(), a, a + L.k.args.size());
            args.resize((size_t)(k + 1) * it->second.stride, 0);
        }
        G.k = it->second.bind(Geo(dim3(k0.grid[0], K), dim3(k0.block[0], k0.block[1], k0.block[2]), k0.lds), upload(args.data(), args.size()));
        return G;
    }

    // every launch of the members' programs `prog(member)` zipped: the sampling programs, which run on lane 0 alone
    template <typename Sel>
    std::vector<GLaunch> zip_lane0(Sel&& prog, const char* what) {
        const Program& p0 = prog(*m[0]);
        std::vector<GLaunch> out;
        for (size_t li = 0; li < p0.launches.size(); ++li) {
            const Launch& L0 = p0.launches[li];
            if (L0.lane != 0 || !L0.waits.empty() || L0.k.grid[1] != 1 || L0.k.grid[2] != 1) invalid("agent groups: launch %zu of %s is not a plain lane-0 launch", li, what);
            for (int k = 1; k < K; ++k) {
                const Program& p = prog(*m[k]);
                if (p.launches.size() != p0.launches.size() || p.launches[li].type != L0.type || p.launches[li].grid != L0.grid || p.launches[li].k.fn != L0.k.fn)
                    invalid("agent groups: launch %zu of member %d's %s differs from member 0's", li, k, what);
            }
            out.push_back(zip((int)li, prog));
        }
        return out;
    }

    // ---- fused sampling (fql_group_sample_actions, fql_group_flow_actions): DESIGN.md section 12 ----
    // The workspace of one chunk of n_pad padded rows per member, cached per n_pad like fql_engine::evals: the launches of every member's
    // get_eval(n_pad).prog_os zipped (and of prog_flow, on the first flow call), the group's staging of host rows and of a host result,
    // [K, m, .] packed by the chunk's m <= n_pad rows, and the [K] argument structs of the assemble and extract launches in device
    // memory, rewritten by every chunk (the rows, the seed and the output are the call's).
    struct Sample {
        int n_pad = 0;
        std::vector<GLaunch> os, flow;
        std::vector<GLaunch> q;            // an IFQL group's best-of-N sampler: the members' critic pair (Eval::prog_q) zipped
        float *st_obs = nullptr, *st_noise = nullptr, *st_out = nullptr;
        float* st_goal = nullptr;          // a CFGRL group: staging of host goals
        unsigned char* d_args = nullptr;   // [K] argument structs of the chunk's first launch, then those of its last (arg_bytes())
        Bound assemble, finish;            // those two multi-instance launches over d_args, blockIdx.y = member
        // an IFQL group's best-of-N sampler, over the other layout of d_args: [K] IfqlRepeatArgs, [K] IfqlQinArgs, [K] IfqlSelectArgs
        Bound repeat, qin, select;
    };
    std::map<int, std::unique_ptr<Sample>> samples;
    // The chunks' argument structs travel through a ring of pinned host slots (the copy reads the slot when the stream reaches it): a
    // slot is reused once the event behind its copy has passed.  On the legacy default stream no event is recorded (fql_engine::grp_legacy):
    // such a slot is reused after a device synchronise.
    static constexpr int kArgRing = 32;
    unsigned char* h_args = nullptr;
    hipEvent_t arg_ev[kArgRing] = {};
    char arg_state[kArgRing] = {};   // 0 = free, 1 = behind arg_ev, 2 = on the legacy stream
    int arg_pos = 0;
    // (a slot holds the layout of the group's kind: [K] AssembleArgs and its finishing launch's [K] structs, or its sweep assembly's
    // [K] structs and [K] ExtractArgs; a best-of-N call [K] IfqlRepeatArgs + [K] IfqlQinArgs + [K] IfqlSelectArgs)
    size_t asm_bytes() const { return kind->sampler == GS_SWEEP ? kind->assemble->bytes : sizeof(AssembleArgs); }
    size_t arg_bytes() const {
        const size_t bon = kind->sampler == GS_BEST_OF_N ? sizeof(IfqlRepeatArgs) + sizeof(IfqlQinArgs) + sizeof(IfqlSelectArgs) : 0;
        return (size_t)K * std::max(asm_bytes() + (kind->sampler == GS_SWEEP ? sizeof(ExtractArgs) : kind->finish->bytes), bon);
    }

    Sample& sample_ws(int n_pad, bool flow) {
        std::unique_ptr<Sample>& slot = samples[n_pad];
        if (!slot) {
            auto w = std::make_unique<Sample>();
            const int od = m[0]->cfg.obs_dim, ad = m[0]->cfg.act_dim;
            w->n_pad = n_pad;
            if (kind->sampler != GS_BEST_OF_N)   // (a best-of-N member's workspace has no one-step actor: its calls are the flow and best of N)
                w->os = zip_lane0([&](fql_engine& e) -> Program& { return e.get_eval(n_pad).prog_os; }, "the one-step sampler");
            w->st_obs = (float*)galloc((size_t)K * n_pad * od * sizeof(float));
            w->st_noise = (float*)galloc((size_t)K * n_pad * ad * sizeof(float));
            w->st_out = (float*)galloc((size_t)K * n_pad * ad * sizeof(float));
            w->d_args = (unsigned char*)galloc(arg_bytes());
            w->assemble = bind(fql_assemble_multi_kernel, Geo(dim3((n_pad + 3) / 4, K), dim3(FQL_THREADS), 0), (const AssembleArgs*)w->d_args);
            w->finish = kind->finish->bind(n_pad, ad, K, w->d_args + (size_t)K * sizeof(AssembleArgs));
            slot = std::move(w);
        }
        if (flow && slot->flow.empty())
            slot->flow = zip_lane0([&](fql_engine& e) -> Program& { return e.get_eval(n_pad).prog_flow; }, "the flow sampler");
        return *slot;
    }
    // An IQL-diffusion group's workspace of one chunk of `half` padded rows per member (Sample::n_pad holds the half): the launches of
    // every member's SWEEP program get_eval(2 half, true).prog_flow zipped - it binds its per-row guidance weights from the member's
    // workspace (Eval::cfgs) and takes no issue-time argument, which a device-resident argument array could not follow - between the
    // multi-instance forms of the two launches fql_engine::sample_flow puts around it.  A CFGRL group's is the same with CFGRL's row
    // assembly, which writes both halves - [obs | goal] and [obs | the member's unc_embed row] - and a staging block for host goals.
    Sample& sample_ws_cfg(int half) {
        std::unique_ptr<Sample>& slot = samples[half];
        if (!slot) {
            auto w = std::make_unique<Sample>();
            const int od = m[0]->cfg.obs_dim, ad = m[0]->cfg.act_dim;
            w->n_pad = half;
            w->flow = zip_lane0([&](fql_engine& e) -> Program& { return e.get_eval(2 * half, true).prog_flow; }, "the guidance-sweep sampler");
            w->st_obs = (float*)galloc((size_t)K * half * od * sizeof(float));
            w->st_noise = (float*)galloc((size_t)K * half * ad * sizeof(float));
            w->st_out = (float*)galloc((size_t)K * half * ad * sizeof(float));
            w->d_args = (unsigned char*)galloc(arg_bytes());
            if (kind->goals) w->st_goal = (float*)galloc((size_t)K * half * m[0]->gcfg.goal_dim * sizeof(float));
            w->assemble = kind->assemble->bind(half, K, w->d_args);
            w->finish = k_finish_extract.bind(half, ad, K, w->d_args + (size_t)K * asm_bytes());
            slot = std::move(w);
        }
        return *slot;
    }
    // An IFQL group's workspace of one chunk of n_pad padded SAMPLE rows per member (num_samples rows per observation): the flow
    // workspace above - the same member workspace get_eval(n_pad) serves both calls - with the members' critic pair zipped and the
    // multi-instance forms of the three launches fql_engine::sample_best_of_n puts around the two programs.  The staging blocks hold
    // what a chunk needs: <= n_pad / N observations, <= n_pad noise rows.  select's grid covers the most observations a chunk of
    // n_pad sample rows can hold; its workgroups past a chunk's own count return at once.
    Sample& sample_ws_bon(int n_pad) {
        Sample& w = sample_ws(n_pad, true);
        if (w.q.empty()) {
            const int N = m[0]->num_samples;
            w.q = zip_lane0([&](fql_engine& e) -> Program& { return e.get_eval(n_pad).prog_q; }, "the best-of-N critic pair");
            const unsigned char* d = w.d_args;
            w.repeat = bind(fql_ifql_repeat_multi_kernel, Geo(dim3((n_pad + 3) / 4, K), dim3(FQL_THREADS), 0), (const IfqlRepeatArgs*)d);
            d += (size_t)K * sizeof(IfqlRepeatArgs);
            w.qin = bind(fql_ifql_qin_multi_kernel, Geo(dim3((n_pad + 3) / 4, K), dim3(FQL_THREADS), 0), (const IfqlQinArgs*)d);
            d += (size_t)K * sizeof(IfqlQinArgs);
            w.select = bind(fql_ifql_select_multi_kernel, Geo(dim3((std::max(1, n_pad / N) + 3) / 4, K), dim3(FQL_THREADS), 0), (const IfqlSelectArgs*)d);
        }
        return w;
    }
    // launches of one fused sampling call on a single chunk, counted from the built program: assemble, the zipped launches, the
    // finishing launch (a best-of-N call: repeat, the flow, qin, the critic pair, select)
    int64_t sample_launches(bool flow) {
        if (kind->sampler == GS_SWEEP) return 2 + (int64_t)sample_ws_cfg(16).flow.size();
        if (kind->sampler == GS_BEST_OF_N && !flow) {
            Sample& w = sample_ws_bon(pad16(m[0]->num_samples));
            return 3 + (int64_t)w.flow.size() + (int64_t)w.q.size();
        }
        Sample& w = sample_ws(16, flow);
        return 2 + (int64_t)(flow ? w.flow : w.os).size();
    }
    unsigned char* arg_slot() {
        if (!h_args) {
            HIP_CHECK(hipHostMalloc((void**)&h_args, kArgRing * arg_bytes()));
            for (hipEvent_t& e : arg_ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        arg_pos = (arg_pos + 1) % kArgRing;
        if (arg_state[arg_pos] == 1) HIP_CHECK(hipEventSynchronize(arg_ev[arg_pos]));
        else if (arg_state[arg_pos] == 2) {
            HIP_CHECK(hipDeviceSynchronize());
            for (char& st : arg_state) if (st == 2) st = 0;
        }
        arg_state[arg_pos] = 0;
        return h_args + (size_t)arg_pos * arg_bytes();
    }
    // rows [start, start + mm) of every member's block of n rows of width w, as one copy over the member stride (a plain copy where
    // both sides are packed)
    void copy_rows(float* dst, size_t dstride, const float* src, size_t sstride, size_t width, hipMemcpyKind kind, hipStream_t s) {
        if (dstride == width && sstride == width) HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)K * width * sizeof(float), kind, s));
        else HIP_CHECK(hipMemcpy2DAsync(dst, dstride * sizeof(float), src, sstride * sizeof(float), width * sizeof(float), (size_t)K, kind, s));
    }
    struct Rows { const float* p; size_t stride; };   // member i's rows of the chunk: p + i * stride
    Rows chunk_rows(const float* src, bool dev, float* staging, int w, int n, int start, int mm, hipStream_t s) {
        if (!src) return Rows{nullptr, 0};
        if (dev) return Rows{src + (size_t)start * w, (size_t)n * w};   // device rows are read where they are
        copy_rows(staging, (size_t)mm * w, src + (size_t)start * w, (size_t)n * w, (size_t)mm * w, hipMemcpyHostToDevice, s);
        return Rows{staging, (size_t)mm * w};
    }
    // One fused sampling call (the caller has ordered `s`: enter()): per chunk of <= 4096 rows per member - the member's own chunks, so
    // that a seeded draw is keyed as fql_engine::eval_rows keys it, (member's key, seed_i + start) - assemble-multi, the zipped launches of
    // the members' program, extract-multi, as direct launches on s.  observations [K, n, od], noise [K, n, ad] or null, out [K, n, ad]:
    // host or device each.  A host result is copied out and waited for per chunk.
    // Members whose actor reads the observation alone (fql_engine::actor_on_obs): assemble-multi of [obs | 0] with the seed unshifted, the
    // zipped launches of the actor's forward, then the kind's finishing launch (SampleFinish), which draws the noise under the member's
    // own row numbers (row0 = start) and writes the actions where extract-multi would.
    void sample(bool flow, const float* obs, const float* noise, const uint64_t* seeds, float temperature, int n, float* out, hipStream_t s) {
        const int od = m[0]->cfg.obs_dim, ad = m[0]->cfg.act_dim;
        const bool on_obs = m[0]->actor_on_obs();
        const bool dev_obs = fql_engine::is_device_ptr(obs), dev_z = noise && fql_engine::is_device_ptr(noise), dev_out = fql_engine::is_device_ptr(out);
        for (int start = 0; start < n; start += 4096) {
            const int mm = std::min(4096, n - start);
            Sample& w = sample_ws(pad16(mm), flow);
            const Rows o = chunk_rows(obs, dev_obs, w.st_obs, od, n, start, mm, s);
            const Rows z = chunk_rows(noise, dev_z, w.st_noise, ad, n, start, mm, s);
            unsigned char* slot = arg_slot();
            AssembleArgs* aa = (AssembleArgs*)slot;
            for (int i = 0; i < K; ++i) {
                fql_engine& e = *m[i];
                fql_engine::Eval& ev = e.get_eval(w.n_pad);
                const ChunkRows r{z.p ? z.p + i * z.stride : nullptr, dev_out ? out + ((size_t)i * n + start) * ad : w.st_out + (size_t)i * mm * ad,
                                  seeds ? seeds[i] : 0, mm, start, temperature};
                if (on_obs)
                    aa[i] = AssembleArgs{o.p + i * o.stride, nullptr, ev.X, e.seed, r.seed, mm, w.n_pad, od, 0, e.nets[NET_BC].in_p()};   // [obs | 0]
                else
                    aa[i] = AssembleArgs{o.p + i * o.stride, r.z, flow ? ev.Xf : ev.X, e.seed, r.seed + (uint64_t)start, mm, w.n_pad, od, ad,
                                         flow ? e.nets[NET_BC].in_p() : e.nets[NET_OS].in_p()};
                kind->finish->fill(slot + (size_t)K * sizeof(AssembleArgs), i, e, ev, flow, r);
            }
            issue_chunk(w, slot, flow ? w.flow : w.os, !dev_obs || (noise && !dev_z), dev_out ? nullptr : out, n, start, mm, s);
        }
    }
    // The tail of a chunk of either sampler: the slot's argument structs to the device with the ring's event behind them, the wait that
    // ends the borrowing of host inputs (host rows - and weights - are the caller's again when the call returns), the assemble launch,
    // the zipped launches, the finishing launch, and a host result (host_out: the call's `out`, [K, n, ad]) copied out and waited for.
    void issue_chunk(Sample& w, const unsigned char* slot, std::vector<GLaunch>& zipped, bool host_inputs, float* host_out, int n, int start, int mm,
                     hipStream_t s) {
        issue_chunk(w, slot, host_inputs, host_out, n, start, mm, s, [&] {
            launch_bound(w.assemble, w.assemble.args.data(), s);
            for (GLaunch& G : zipped) launch_bound(G.k, G.k.args.data(), s);
            launch_bound(w.finish, w.finish.args.data(), s);
        });
    }
    // (the same with the chunk's launches as a callable: an IFQL group's best-of-N chunk is five groups of launches, not three)
    template <typename Launches>
    void issue_chunk(Sample& w, const unsigned char* slot, bool host_inputs, float* host_out, int n, int start, int mm, hipStream_t s, Launches&& launches) {
        const int ad = m[0]->cfg.act_dim;
        HIP_CHECK(hipMemcpyAsync(w.d_args, slot, arg_bytes(), hipMemcpyHostToDevice, s));
        if (s == hipStreamLegacy) arg_state[arg_pos] = 2;
        else { HIP_CHECK(hipEventRecord(arg_ev[arg_pos], s)); arg_state[arg_pos] = 1; }
        if (host_inputs) HIP_CHECK(hipStreamSynchronize(s));
        launches();
        HIP_CHECK(hipGetLastError());
        if (host_out) {
            copy_rows(host_out + (size_t)start * ad, (size_t)n * ad, w.st_out, (size_t)mm * ad, (size_t)mm * ad, hipMemcpyDeviceToHost, s);
            HIP_CHECK(hipStreamSynchronize(s));
        }
    }

    // An IQL-diffusion group (fql_iqld_group_sample_actions): fql_iqld_sample_actions_cfgs of every member in one fused call.  Per chunk
    // of <= 2048 observations per member - the member's own chunks, row numbers and seed key (fql_engine::sample_flow) -
    // fql_bc_assemble_multi_kernel, each member's chunk of `cfgs` [K, n] (host: checked finite here; or device) copied into the buffer
    // its sweep program reads with 0 behind it, the zipped launches, extract-multi.
    // A CFGRL group (fql_cfgrl_group_sample_actions): fql_cfgrl_sample_actions_cfgs of every member the same way, with `goals` [K, n, G]
    // beside the observations and fql_cfgrl_assemble_multi_kernel, whose unconditional half reads each member's own unc_embed leaf.
    void sample_cfg(const float* obs, const float* goals, const float* noise, const uint64_t* seeds, const float* cfgs, int n, float* out, hipStream_t s) {
        const int od = m[0]->cfg.obs_dim, ad = m[0]->cfg.act_dim, Gd = kind->goals ? m[0]->gcfg.goal_dim : 0;
        const bool dev_obs = fql_engine::is_device_ptr(obs), dev_z = noise && fql_engine::is_device_ptr(noise), dev_out = fql_engine::is_device_ptr(out);
        const bool dev_c = fql_engine::is_device_ptr(cfgs), dev_g = !Gd || fql_engine::is_device_ptr(goals);
        if (!dev_c)
            for (size_t i = 0; i < (size_t)K * n; ++i)
                if (!std::isfinite(cfgs[i])) invalid("cfgs[%zu][%zu] = %g: every guidance weight must be finite", i / n, i % n, (double)cfgs[i]);
        for (int start = 0; start < n; start += 2048) {
            const int mm = std::min(2048, n - start), half = pad16(mm);
            Sample& w = sample_ws_cfg(half);
            const Rows o = chunk_rows(obs, dev_obs, w.st_obs, od, n, start, mm, s);
            const Rows z = chunk_rows(noise, dev_z, w.st_noise, ad, n, start, mm, s);
            const Rows gl = Gd ? chunk_rows(goals, dev_g, w.st_goal, Gd, n, start, mm, s) : Rows{nullptr, 0};
            unsigned char* slot = arg_slot();
            for (int i = 0; i < K; ++i) {
                fql_engine& e = *m[i];
                fql_engine::Eval& ev = e.get_eval(2 * half, true);
                const ChunkRows r{z.p ? z.p + i * z.stride : nullptr, dev_out ? out + ((size_t)i * n + start) * ad : w.st_out + (size_t)i * mm * ad,
                                  seeds ? seeds[i] : 0, mm, start, 1.0f};
                kind->assemble->fill(slot, i, e, ev, o.p + i * o.stride, Gd ? gl.p + i * gl.stride : nullptr, half, r);
                k_finish_extract.fill(slot + (size_t)K * asm_bytes(), i, e, ev, true, r);
                HIP_CHECK(hipMemcpyAsync(ev.cfgs, cfgs + (size_t)i * n + start, (size_t)mm * sizeof(float), hipMemcpyDefault, s));
                if (half > mm) HIP_CHECK(hipMemsetAsync(ev.cfgs + mm, 0, (size_t)(half - mm) * sizeof(float), s));
            }
            issue_chunk(w, slot, w.flow, !dev_obs || (noise && !dev_z) || !dev_c || !dev_g, dev_out ? nullptr : out, n, start, mm, s);
        }
    }

    // An IFQL group (fql_ifql_group_sample_actions): fql_sample_actions of every member - best of num_samples - in one fused call.  Per
    // chunk of <= 4096 SAMPLE rows per member - the member's own chunks (fql_engine::sample_chunks with SampleSpec{0, N}), its row numbers
    // (row0 = start N) and its seed key, so a seeded draw is the member's own - repeat-multi, the zipped launches of the members' Euler
    // flow, qin-multi, the zipped launches of their critic pair, select-multi, which writes the chunk's actions where the caller's `out`
    // is device memory and into the staging block where it is not.  noise: [K, n, N, ad] or null.
    void sample_bon(const float* obs, const float* noise, const uint64_t* seeds, int n, float* out, hipStream_t s) {
        const int od = m[0]->cfg.obs_dim, ad = m[0]->cfg.act_dim, ap = pad16(ad), N = m[0]->num_samples;
        const bool dev_obs = fql_engine::is_device_ptr(obs), dev_z = noise && fql_engine::is_device_ptr(noise), dev_out = fql_engine::is_device_ptr(out);
        const int per = std::max(1, 4096 / N);
        for (int start = 0; start < n; start += per) {
            const int mm = std::min(per, n - start);
            Sample& w = sample_ws_bon(pad16(mm * N));
            const Rows o = chunk_rows(obs, dev_obs, w.st_obs, od, n, start, mm, s);
            const Rows z = chunk_rows(noise, dev_z, w.st_noise, N * ad, n, start, mm, s);
            unsigned char* slot = arg_slot();
            IfqlRepeatArgs* ra = (IfqlRepeatArgs*)slot;
            IfqlQinArgs* qa = (IfqlQinArgs*)(slot + (size_t)K * sizeof(IfqlRepeatArgs));
            IfqlSelectArgs* sa = (IfqlSelectArgs*)(slot + (size_t)K * (sizeof(IfqlRepeatArgs) + sizeof(IfqlQinArgs)));
            for (int i = 0; i < K; ++i) {
                fql_engine& e = *m[i];
                fql_engine::Eval& ev = e.get_eval(w.n_pad);
                const float* oi = o.p + i * o.stride;
                ra[i] = IfqlRepeatArgs{oi, z.p ? z.p + i * z.stride : nullptr, ev.Xf, e.seed, seeds ? seeds[i] : 0, mm, N, w.n_pad, od, ad,
                                       e.nets[NET_BC].in_p(), start * N};
                qa[i] = IfqlQinArgs{oi, ev.tgt, ev.Xq, mm, N, w.n_pad, od, ad, ap, e.nets[NET_C0].in_p()};
                sa[i] = IfqlSelectArgs{ev.p_q[0].out, ev.p_q[1].out, ev.tgt, dev_out ? out + ((size_t)i * n + start) * ad : w.st_out + (size_t)i * mm * ad,
                                       mm, N, ad, ap};
            }
            issue_chunk(w, slot, !dev_obs || (noise && !dev_z), dev_out ? nullptr : out, n, start, mm, s, [&] {
                launch_bound(w.repeat, w.repeat.args.data(), s);
                for (GLaunch& G : w.flow) launch_bound(G.k, G.k.args.data(), s);
                launch_bound(w.qin, w.qin.args.data(), s);
                for (GLaunch& G : w.q) launch_bound(G.k, G.k.args.data(), s);
                launch_bound(w.select, w.select.args.data(), s);
            });
        }
    }

    // ---- ordering of a group call (update or sampling) against the group's last call and against the members' own work ----
    // The stream the call runs on, ordered (0) behind the group's last call where that ran on another stream (the caller's, then the
    // group's own, or the reverse) and (1) behind everything submitted through a member since the last group call.
    hipStream_t enter(void* stream) {
        const hipStream_t s = stream ? (hipStream_t)stream : lanes[0];
        if (last && last != s) HIP_CHECK(last == hipStreamLegacy ? hipDeviceSynchronize() : hipStreamWaitEvent(s, ev_done, 0));
        last = s;
        for (fql_handle h : m) {
            if (!h->grp_touched) continue;
            h->aql_drain();
            HIP_CHECK(hipEventRecord(ev_in, h->stream));
            HIP_CHECK(hipStreamWaitEvent(s, ev_in, 0));
            h->grp_touched = false;
        }
        return s;
    }
    // The call is enqueued on s: every member entry point waits for it from here on (fql_engine::group_fence / group_order).  No event is
    // recorded on the legacy default stream (fql_engine::grp_legacy): waits for such a call synchronise the device.  host_wait: the call
    // hands a result to host memory and returns when it is there.
    void leave(hipStream_t s, bool host_wait) {
        const bool legacy = s == hipStreamLegacy;
        if (!legacy) HIP_CHECK(hipEventRecord(ev_done, s));
        for (fql_handle h : m) { h->grp_pending = true; h->grp_legacy = legacy; h->grp_touched = false; }
        if (host_wait) HIP_CHECK(legacy ? hipDeviceSynchronize() : hipEventSynchronize(ev_done));
    }
    bool member_began() const {
        for (fql_handle h : m) if (h->began) return true;
        return false;
    }

    // the fused program as ONE graph with the lanes, forks, joins and cross-lane events of a member's own
    void capture(GProgram& p) {
        capture_graph(lanes[0], [&] { issue_lanes(p, lanes[0], lanes, true, [&](GLaunch& G, hipStream_t s) { launch_bound(G.k, G.k.args.data(), s); }); }, p.graph, p.exec);
    }

    void release() {
        if (lanes[0]) hipStreamSynchronize(lanes[0]);
        if (last == hipStreamLegacy) hipDeviceSynchronize();
        if (ev_done) hipEventSynchronize(ev_done);
        for (fql_handle h : m) { h->group = nullptr; h->grp_pending = h->grp_legacy = false; h->grp_done = nullptr; h->grp_touched = true; }
        for (GProgram& p : progs) {
            if (p.exec) hipGraphExecDestroy(p.exec);
            if (p.graph) hipGraphDestroy(p.graph);
            destroy_lane_events(p);
        }
        for (hipEvent_t e : {ev_in, ev_done}) if (e) hipEventDestroy(e);
        for (hipEvent_t e : arg_ev) if (e) hipEventDestroy(e);
        if (h_args) hipHostFree(h_args);
        for (void* p : allocs) hipFree(p);
        if (d_idx) hipFree(d_idx);
        for (hipStream_t s : lanes) if (s) hipStreamDestroy(s);
    }
};

namespace {
// The body of a group entry point: FQL_OK, or the code of what it threw with the message where fql_last_error(NULL) reads it
#define GROUP_TRY(...)                                     \
    try {                                                  \
        __VA_ARGS__;                                       \
        return FQL_OK;                                     \
    } catch (const Invalid& e) {                           \
        g_create_error = e.msg;                            \
        return FQL_E_INVALID;                              \
    } catch (const HipError& e) {                          \
        g_create_error = e.msg;                            \
        return FQL_E_HIP;                                  \
    } catch (const std::exception& e) {                    \
        g_create_error = e.what();                         \
        return FQL_E_HIP;                                  \
    }
// A group call on a group of another kind: FQL_E_STATE, naming the call of the group's own kind that serves it
bool group_wrong_kind(fql_group g, AgentKind kind, const char* fn, GroupCall c) {
    if (g->kind->kind == kind) return false;
    g_create_error = std::string(fn) + " is not available on a group of " + g->m[0]->desc().name + " agents (" + g->kind->calls[c] + ")";
    return true;
}
// the first line of an entry point `fn` that serves groups of `kind`
#define GROUP_ENTER(g, kind, fn, call)                                                                \
    do {                                                                                              \
        if (!(g)) { g_create_error = std::string(fn) + ": NULL group"; return FQL_E_INVALID; }        \
        if (group_wrong_kind((g), (kind), (fn), (call))) return FQL_E_STATE;                          \
    } while (0)

// the members' restrictions and the structural identity of their programs (`fn`: the create call)
void group_check(const char* fn, const GroupKind& kind, const fql_handle* members, int k) {
    if (!members || k <= 0) invalid("%s: members must be a non-empty array (k = %d)", fn, k);
    for (int i = 0; i < k; ++i) {
        fql_handle h = members[i];
        if (!h) invalid("%s: member %d is NULL", fn, i);
        for (int j = 0; j < i; ++j) if (members[j] == h) invalid("%s: member %d appears twice", fn, i);
        if (h->group) invalid("%s: member %d already belongs to a group", fn, i);
        if (h->visual) invalid("%s: member %d has an encoder (groups take state agents only)", fn, i);
        if (h->cfg.precision != 0) invalid("%s: member %d has precision %d (groups take fp32 members only)", fn, i, h->cfg.precision);
        if (h->began) invalid("%s: member %d is between fql_update_begin and fql_update_end", fn, i);
        if (!kind.same_structure(*h, *members[0])) invalid("%s: member %d's config differs from member 0's in more than seed and %s", fn, i, kind.free_fields);
        if (h->B != members[0]->B) invalid("%s: member %d has batch size %d, member 0 has %d", fn, i, h->B, members[0]->B);
        for (int pi = 0; pi < kind.programs; ++pi) {
            const Program& p = h->*k_group_programs[pi], &p0 = members[0]->*k_group_programs[pi];
            require_graph(p);
            if (p.launches.size() != p0.launches.size()) invalid("%s: member %d's update has %zu launches, member 0's %zu", fn, i, p.launches.size(), p0.launches.size());
            for (size_t li = 0; li < p.launches.size(); ++li) {
                const Launch &L = p.launches[li], &L0 = p0.launches[li];
                if (L.type != L0.type || L.lane != L0.lane || L.grid != L0.grid || L.waits != L0.waits || L.record_after != L0.record_after)
                    invalid("%s: launch %zu of member %d differs from member 0's (type %d/%d, lane %d/%d, grid %d/%d)", fn, li, i, (int)L.type,
                            (int)L0.type, L.lane, L0.lane, L.grid, L0.grid);
                if (L.type == OP_WFRAG && h->wfrag_grid != members[0]->wfrag_grid) invalid("%s: member %d's weight-copy launch differs", fn, i);
            }
        }
    }
}

// a group of `which` members: the kind's create call
int group_create(AgentKind which, const fql_handle* members, int k, fql_group* out) {
    const GroupKind& kind = k_group_kinds[(int)which];
    const char* fn = kind.create;
    if (!out) { g_create_error = std::string(fn) + ": out must not be NULL"; return FQL_E_INVALID; }
    *out = nullptr;
    for (int i = 0; members && i < k; ++i)
        if (members[i] && members[i]->kind != which) {
            const char* grouped_by = k_group_kinds[(int)members[i]->kind].grouped_by;
            g_create_error = std::string(fn) + ": member " + std::to_string(i) + " is " + members[i]->desc().label + " (" + kind.takes + (grouped_by ? grouped_by : "") + ")";
            return FQL_E_STATE;
        }
    struct Release { void operator()(fql_group_s* g) const { g->release(); delete g; } };
    GROUP_TRY({
        std::unique_ptr<fql_group_s, Release> g(new fql_group_s());
        group_check(fn, kind, members, k);
        g->m.assign(members, members + k);
        g->kind = &kind;
        g->K = k;
        g->B = members[0]->B;
        for (fql_handle h : g->m) { h->aql_drain(); HIP_CHECK(hipStreamSynchronize(h->stream)); }
        for (int pi = 0; pi < kind.programs; ++pi) {
            GProgram& gp = g->progs[pi];
            Program fql_engine::* pp = k_group_programs[pi];
            const size_t n = (g->m[0]->*pp).launches.size();
            for (size_t li = 0; li < n; ++li)
                for (int i = 1; i < k; ++i) {
                    const Bound &a = (g->m[i]->*pp).launches[li].k, &b = (g->m[0]->*pp).launches[li].k;
                    if (a.fn != b.fn || std::memcmp(a.grid, b.grid, sizeof a.grid) || std::memcmp(a.block, b.block, sizeof a.block) || a.lds != b.lds)
                        invalid("%s: launch %zu of member %d runs another kernel or shape than member 0's", fn, li, i);
                }
            for (size_t li = 0; li < n; ++li) {
                const Bound& k0 = (g->m[0]->*pp).launches[li].k;
                if (k0.grid[1] != 1 || k0.grid[2] != 1) invalid("%s: launch %zu has a 2-D grid: not groupable", fn, li);   // (grid y is the member)
                gp.launches.push_back(g->zip((int)li, [pp](fql_engine& e) -> Program& { return e.*pp; }));
                gp.lane_used[gp.launches.back().lane] = true;
            }
        }
        for (int l = 0; l < FQL_LANES; ++l) HIP_CHECK(hipStreamCreateWithFlags(&g->lanes[l], hipStreamNonBlocking));
        for (hipEvent_t* e : {&g->ev_in, &g->ev_done}) HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        HIP_CHECK(hipMalloc((void**)&g->d_idx, (size_t)k * g->B * sizeof(int64_t)));
        if (kind.goals) g->d_mask = (unsigned char*)g->galloc((size_t)k * g->B);
        for (int pi = 0; pi < kind.programs; ++pi) g->capture(g->progs[pi]);
        for (fql_handle h : g->m) { h->group = g.get(); h->grp_done = g->ev_done; h->grp_pending = false; h->grp_touched = true; }
        *out = g.release();
    });
}

// What one fused update runs beside its rows: the group's program for the step's kind; a goal kind's `do_cfg`, [k][B] bytes, host or
// device, or NULL = each member's Philox mask; balanced (fql_sac_group_update_balanced): every member's source is its two-source one
// (fql_engine::source_balanced: B / 2 rows of its dataset, B / 2 of its own replay ring), idx and idx_rb [k][B / 2] each, both or
// neither, host or device, staged into each member's index buffer as its own call stages them.
struct GroupStep {
    int prog = fql_group_s::FULL;
    const unsigned char* do_cfg = nullptr;
    bool balanced = false;
    const int64_t* idx_rb = nullptr;
};
// One fused update of every member.  fn: the entry point, for its messages.  infos: [k][the members' num_info(), or GroupKind::infos] out of each
// member's info buffer (fql_engine::info_src).  A goal kind: every member's goal source (CfgrlSrc: its goal table, its mixture thresholds and its
// rows of do_cfg) is set beside its dataset source, as fql_cfgrl_update_from_dataset sets them.  Every member is checked before any
// member's source is written: a refusal leaves every member where it was.
int group_update(fql_group g, const char* fn, const int64_t* idx, int batch_size, float* infos, void* stream, const GroupStep& st = GroupStep()) {
    GROUP_TRY({
        if (batch_size != g->B) invalid("%s: batch_size %d does not match the members' %d", fn, batch_size, g->B);
        if (g->member_began()) { g_create_error = std::string(fn) + ": a member is between fql_update_begin and fql_update_end"; return FQL_E_STATE; }
        if (st.balanced) {
            if (g->B % 2) invalid("%s: balanced sampling draws batch_size // 2 rows from each source: batch_size %d must be even", fn, g->B);
            if (!idx != !st.idx_rb) invalid("%s: balanced sampling: give both index arrays or neither", fn);
            for (int i = 0; i < g->K; ++i) {
                const fql_engine& e = *g->m[i];
                if (e.ds_size <= 0 || !e.ds_obs) invalid("%s: member %d has no training dataset uploaded", fn, i);
                if (e.rb_cap <= 0) invalid("%s: member %d has no replay ring (fql_replay_create)", fn, i);
                if (e.rb_size <= 0) invalid("%s: member %d's replay ring is empty (the reference would draw randint(0), a ValueError)", fn, i);
            }
        }
        for (int i = 0; g->kind->goals && i < g->K; ++i)
            if (!g->m[i]->ds_final) invalid("%s: member %d has no goal table (fql_cfgrl_dataset_goals after fql_dataset_upload)", fn, i);
        const hipStream_t s = g->enter(stream);
        const unsigned char* mask = st.do_cfg;
        if (mask && !fql_engine::is_device_ptr(mask)) {   // (borrowed for the call only: the wait is the indices' below, or its own)
            HIP_CHECK(hipMemcpyAsync(g->d_mask, mask, (size_t)g->K * g->B, hipMemcpyHostToDevice, s));
            if (!idx || fql_engine::is_device_ptr(idx)) HIP_CHECK(hipStreamSynchronize(s));
            mask = g->d_mask;
        }
        const int64_t* rows = idx;
        if (idx && !st.balanced && !fql_engine::is_device_ptr(idx)) {
            HIP_CHECK(hipMemcpyAsync(g->d_idx, idx, (size_t)g->K * g->B * sizeof(int64_t), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));   // (host indices are borrowed for the call only)
            rows = g->d_idx;
        }
        for (int i = 0; i < g->K; ++i) {
            const int64_t* ri = rows ? rows + (size_t)i * g->B : nullptr;
            if (g->kind->goals) g->m[i]->cfgrl_source_from_dataset(ri, g->B, 0, 0, nullptr, mask ? mask + (size_t)i * g->B : nullptr, s);
            else if (st.balanced) g->m[i]->source_balanced(idx ? idx + (size_t)i * (g->B / 2) : nullptr, st.idx_rb ? st.idx_rb + (size_t)i * (g->B / 2) : nullptr, nullptr, g->B, nullptr, s);
            else g->m[i]->source_from_dataset(ri, g->B, 0, 0, nullptr, s);
        }
        HIP_CHECK(hipGraphLaunch(g->progs[st.prog].exec, s));
        const size_t n_info = (size_t)(g->kind->infos ? g->kind->infos : g->m[0]->num_info());
        for (int i = 0; infos && i < g->K; ++i)
            HIP_CHECK(hipMemcpyAsync(infos + i * n_info, g->m[i]->info_src(), n_info * sizeof(float), hipMemcpyDefault, s));
        g->leave(s, infos && !fql_engine::is_device_ptr(infos));
    });
}

// Launches counted from the built programs, each where its out-pointer is given: of the group's fused update programs, in their order,
// and of one fused sampling call and one fused flow call (a sweep kind: its one sampler answers either) on a single chunk
int group_stats(fql_group g, std::initializer_list<int64_t*> programs, int64_t* sample, int64_t* flow) {
    GROUP_TRY({
        int pi = 0;
        for (int64_t* out : programs) {
            if (out) *out = (int64_t)g->progs[pi].launches.size();
            ++pi;
        }
        if (sample) *sample = g->sample_launches(false);
        if (flow) *flow = g->sample_launches(true);
    });
}

// The members' sample_actions (flow: compute_flow_actions) in one fused call, between the update's ordering rules: the chunk loop of
// the group's kind (fql_group_s::sample; best of N: fql_group_s::sample_bon, whose flow call is the plain loop's)
int group_sample(fql_group g, const char* fn, AgentKind kind, bool flow, const float* obs, const float* noise, const uint64_t* seeds, float temperature, int n,
                 float* out, void* stream) {
    GROUP_ENTER(g, kind, fn, flow ? GC_FLOW : GC_SAMPLE);
    GROUP_TRY({
        if (n <= 0) invalid("%s: n must be positive (got %d)", fn, n);
        if (!obs || !out) invalid("%s: observations/out must not be NULL", fn);
        if (flow && !noise) invalid("%s: noises must not be NULL", fn);
        if (!noise && !seeds) invalid("%s: seeds must not be NULL when noises is NULL (one seed per member)", fn);
        if (!(temperature >= 0.0f)) invalid("%s: temperature must be >= 0", fn);
        if (g->member_began()) { g_create_error = std::string(fn) + ": a member is between fql_update_begin and fql_update_end"; return FQL_E_STATE; }
        const hipStream_t s = g->enter(stream);
        if (g->kind->sampler == GS_BEST_OF_N && !flow) g->sample_bon(obs, noise, seeds, n, out, s);
        else g->sample(flow, obs, noise, seeds, temperature, n, out, s);
        // a device result on the group's own stream: the caller has no handle to order its reads against, so finish here (as a member does)
        g->leave(s, !stream && fql_engine::is_device_ptr(out));
    });
}
// The members' per-row guidance sweep (fql_iqld_sample_actions_cfgs, fql_cfgrl_sample_actions_cfgs) in one fused call:
// fql_group_s::sample_cfg between the update's ordering rules.  goals: a goal kind's [k][n][G], which its conditional pass reads
int group_sample_cfg(fql_group g, const char* fn, AgentKind kind, const float* observations, const float* goals, int n, const float* noises,
                     const uint64_t* seeds, const float* cfgs, float* out, void* stream) {
    GROUP_ENTER(g, kind, fn, GC_SAMPLE);
    GROUP_TRY({
        if (n <= 0) invalid("%s: n must be positive (got %d)", fn, n);
        if (!observations || !out) invalid("%s: observations/out must not be NULL", fn);
        if (g->kind->goals && !goals) invalid("%s: goals must not be NULL (the conditional pass reads them: agents/cfgrl.py:93)", fn);
        if (!cfgs) invalid("%s: cfgs must not be NULL (one guidance weight per member and row)", fn);
        if (!noises && !seeds) invalid("%s: seeds must not be NULL when noises is NULL (one seed per member)", fn);
        if (g->member_began()) { g_create_error = std::string(fn) + ": a member is between fql_update_begin and fql_update_end"; return FQL_E_STATE; }
        const hipStream_t s = g->enter(stream);
        g->sample_cfg(observations, goals, noises, seeds, cfgs, n, out, s);
        g->leave(s, !stream && fql_engine::is_device_ptr(out));
    });
}
}  // namespace

extern "C" {

int fql_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::FQL, members, k, out); }
int fql_rebrac_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::REBRAC, members, k, out); }
int fql_iqld_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::IQLD, members, k, out); }
int fql_ifql_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::IFQL, members, k, out); }
int fql_iql_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::IQL, members, k, out); }
int fql_cfgrl_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::CFGRL, members, k, out); }
int fql_sac_group_create(const fql_handle* members, int k, fql_group* out) { return group_create(AgentKind::SAC, members, k, out); }

// Diagnostic only (not in include/fql_amd.h, beside fql_debug_plan): where each launch of an update program takes its tasks from, as int32 words
//   [words (this one included), capacities of the argument form of a side-lane launch: GEMM-tile, weight-gradient, LayerNorm-backward, loss / metric
//    tasks, launches], then per launch one word:
//   0 = the launch has no task table, 1 = its tasks are a table in HBM, 2 = they are the kernel argument (FQL_KERNARG_TASKS, fql_kernels.h find_front)
// of the group `g`'s fused program when g is given, else of the handle's prog_full (same refusals as fql_debug_plan).  Prefix reads as there.
int fql_debug_task_forms(fql_handle h, fql_group g, void* out, size_t bytes) {
    if ((!h && !g) || (bytes && !out) || bytes % sizeof(int32_t)) return FQL_E_INVALID;
    if (!g && (h->visual || !h->prog_full.exec || h->prog_full.launches.empty())) return FQL_E_STATE;
    auto form = [](const Launch& L) { return !is_table_launch(L.type) ? 0 : L.ka ? 2 : 1; };
    std::vector<int32_t> w{0, FQL_KA_GEMM, FQL_KA_WGRAD, FQL_KA_LN, FQL_KA_MISC, 0};
    if (g) for (const GLaunch& G : g->progs[fql_group_s::FULL].launches) w.push_back(G.form);
    else for (const Launch& L : h->prog_full.launches) w.push_back(form(L));
    w[5] = (int32_t)w.size() - 6;
    w[0] = (int32_t)w.size();
    if (bytes > w.size() * sizeof(int32_t)) return FQL_E_INVALID;
    if (bytes) std::memcpy(out, w.data(), bytes);
    return FQL_OK;
}

// Diagnostic only (not in include/fql_amd.h, beside fql_debug_task_forms): the fences of the kernel packets of an update program on the engine's own
// queues, as int32 words
//   [words (this one included), 1 if every launch binds a kernel of l1_independent_kernel's table (and none has an issue-time word) else 0,
//    1 if FQL_AQL_ACQUIRE was set when the engine was created else 0, kernel packets], then per kernel packet, lane by lane in queue order:
//   lane, acquire scope, release scope (hsa_fence_scope_t: 0 none, 1 agent, 2 system) - read back from the packet headers build_aql wrote
// of the handle's prog_full (no packets before its first update on the engine's own stream, or where the AQL path is off), or of the group `g`'s
// fused program when g is given: a group runs its captured graph, so it has the table word and no packets.  Prefix reads as there.
int fql_debug_aql_fences(fql_handle h, fql_group g, void* out, size_t bytes) {
    if ((!h && !g) || (bytes && !out) || bytes % sizeof(int32_t)) return FQL_E_INVALID;
    if (!g && (h->visual || !h->prog_full.exec || h->prog_full.launches.empty())) return FQL_E_STATE;
    std::vector<int32_t> w{0, 0, 0, 0};
    if (g) {
        bool all = !g->progs[fql_group_s::FULL].launches.empty();
        for (const GLaunch& G : g->progs[fql_group_s::FULL].launches) all = all && l1_independent_kernel(G.k.fn);
        w[1] = all;
        w[2] = g->m.empty() ? 0 : (int32_t)g->m[0]->aql_acquire;
    } else {
        w[1] = fql_engine::l1_independent(h->prog_full);
        w[2] = h->aql_acquire;
        const AqlProgram& ap = h->prog_full.aql;
        if (ap.ok)
            for (int l = 0; l < FQL_AQL_LANES; ++l)
                for (const AqlPacket& p : ap.lane[l]) {
                    if (p.barrier) continue;
                    const uint32_t hdr = p.w[0] & 0xFFFFu;
                    w.push_back(l);
                    w.push_back((int32_t)((hdr >> HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) & 3u));
                    w.push_back((int32_t)((hdr >> HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE) & 3u));
                }
    }
    w[3] = ((int32_t)w.size() - 4) / 3;
    w[0] = (int32_t)w.size();
    if (bytes > w.size() * sizeof(int32_t)) return FQL_E_INVALID;
    if (bytes) std::memcpy(out, w.data(), bytes);
    return FQL_OK;
}

int fql_group_destroy(fql_group g) {
    if (!g) return FQL_OK;
    g->release();
    delete g;
    return FQL_OK;
}

// The kind's update_from_dataset of every member in one fused update: the zip of their program of the step's kind
int fql_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* info13xk, void* stream) {
    const char* fn = "fql_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::FQL, fn, GC_UPDATE);
    return group_update(g, fn, idx, batch_size, info13xk, stream);
}
int fql_rebrac_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, int full_update, float* info13xk, void* stream) {
    const char* fn = "fql_rebrac_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::REBRAC, fn, GC_UPDATE);
    GroupStep st;
    st.prog = full_update ? fql_group_s::FULL : fql_group_s::CRITIC;
    return group_update(g, fn, idx, batch_size, info13xk, stream, st);
}
int fql_iqld_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, int update_critic, int update_actor, float* info21xk, void* stream) {
    const char* fn = "fql_iqld_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::IQLD, fn, GC_UPDATE);
    GroupStep st;
    st.prog = update_critic ? (update_actor ? fql_group_s::FULL : fql_group_s::CRITIC) : (update_actor ? fql_group_s::ACTOR : fql_group_s::NONE);
    return group_update(g, fn, idx, batch_size, info21xk, stream, st);
}
int fql_ifql_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* info12xk, void* stream) {
    const char* fn = "fql_ifql_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::IFQL, fn, GC_UPDATE);
    return group_update(g, fn, idx, batch_size, info12xk, stream);
}
// (16 infos per member under awr, 19 under ddpgbc)
int fql_iql_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* infoNxk, void* stream) {
    const char* fn = "fql_iql_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::IQL, fn, GC_UPDATE);
    return group_update(g, fn, idx, batch_size, infoNxk, stream);
}
// (behind each member's dataset source and goal source)
int fql_cfgrl_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, const uint8_t* do_cfg, float* info4xk, void* stream) {
    const char* fn = "fql_cfgrl_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::CFGRL, fn, GC_UPDATE);
    GroupStep st;
    st.do_cfg = do_cfg;
    return group_update(g, fn, idx, batch_size, info4xk, stream, st);
}
int fql_sac_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* info14xk, void* stream) {
    const char* fn = "fql_sac_group_update_from_dataset";
    GROUP_ENTER(g, AgentKind::SAC, fn, GC_UPDATE);
    return group_update(g, fn, idx, batch_size, info14xk, stream);
}
// fql_sac_update_balanced of every SAC member in one fused update: the same program behind each member's two-source descriptor
int fql_sac_group_update_balanced(fql_group g, const int64_t* idx_dataset, const int64_t* idx_replay, int batch_size, float* info14xk, void* stream) {
    const char* fn = "fql_sac_group_update_balanced";
    GROUP_ENTER(g, AgentKind::SAC, fn, GC_UPDATE);
    GroupStep st;
    st.balanced = true;
    st.idx_rb = idx_replay;
    return group_update(g, fn, idx_dataset, batch_size, info14xk, stream, st);
}

int fql_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float* out, void* stream) {
    return group_sample(g, "fql_group_sample_actions", AgentKind::FQL, false, observations, noises, seeds, 1.0f, n, out, stream);
}
int fql_group_flow_actions(fql_group g, const float* observations, const float* noises, int n, float* out, void* stream) {
    return group_sample(g, "fql_group_flow_actions", AgentKind::FQL, true, observations, noises, nullptr, 1.0f, n, out, stream);
}
int fql_rebrac_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float temperature,
                                    float* out, void* stream) {
    return group_sample(g, "fql_rebrac_group_sample_actions", AgentKind::REBRAC, false, observations, noises, seeds, temperature, n, out, stream);
}
int fql_ifql_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float* out, void* stream) {
    return group_sample(g, "fql_ifql_group_sample_actions", AgentKind::IFQL, false, observations, noises, seeds, 1.0f, n, out, stream);
}
int fql_ifql_group_flow_actions(fql_group g, const float* observations, const float* noises, int n, float* out, void* stream) {
    return group_sample(g, "fql_ifql_group_flow_actions", AgentKind::IFQL, true, observations, noises, nullptr, 1.0f, n, out, stream);
}
int fql_iql_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float temperature,
                                 float* out, void* stream) {
    return group_sample(g, "fql_iql_group_sample_actions", AgentKind::IQL, false, observations, noises, seeds, temperature, n, out, stream);
}
int fql_sac_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float temperature,
                                 float* out, void* stream) {
    return group_sample(g, "fql_sac_group_sample_actions", AgentKind::SAC, false, observations, noises, seeds, temperature, n, out, stream);
}
int fql_iqld_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, const float* cfgs,
                                  float* out, void* stream) {
    return group_sample_cfg(g, "fql_iqld_group_sample_actions", AgentKind::IQLD, observations, nullptr, n, noises, seeds, cfgs, out, stream);
}
int fql_cfgrl_group_sample_actions(fql_group g, const float* observations, const float* goals, int n, const float* noises, const uint64_t* seeds,
                                   const float* cfgs, float* out, void* stream) {
    return group_sample_cfg(g, "fql_cfgrl_group_sample_actions", AgentKind::CFGRL, observations, goals, n, noises, seeds, cfgs, out, stream);
}

// Launches of the group's fused update programs and of one fused sampling call on a single chunk, counted from the built programs
int fql_group_sample_stats(fql_group g, int flow, int64_t* launches_per_call) {
    GROUP_ENTER(g, AgentKind::FQL, "fql_group_sample_stats", GC_STATS);
    if (!launches_per_call) { g_create_error = "fql_group_sample_stats: launches_per_call must not be NULL"; return FQL_E_INVALID; }
    return group_stats(g, {}, flow ? nullptr : launches_per_call, flow ? launches_per_call : nullptr);
}
int fql_rebrac_group_stats(fql_group g, int64_t* launches_full, int64_t* launches_critic, int64_t* launches_sample) {
    GROUP_ENTER(g, AgentKind::REBRAC, "fql_rebrac_group_stats", GC_STATS);
    return group_stats(g, {launches_full, launches_critic}, launches_sample, nullptr);
}
// (full, critic-only, actor-only, neither)
int fql_iqld_group_stats(fql_group g, int64_t launches[4], int64_t* launches_sample) {
    GROUP_ENTER(g, AgentKind::IQLD, "fql_iqld_group_stats", GC_STATS);
    if (!launches) return group_stats(g, {}, launches_sample, nullptr);
    return group_stats(g, {launches, launches + 1, launches + 2, launches + 3}, launches_sample, nullptr);
}
// (one fused best-of-N and one fused flow call)
int fql_ifql_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample, int64_t* launches_flow) {
    GROUP_ENTER(g, AgentKind::IFQL, "fql_ifql_group_stats", GC_STATS);
    return group_stats(g, {launches_update}, launches_sample, launches_flow);
}
int fql_iql_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample) {
    GROUP_ENTER(g, AgentKind::IQL, "fql_iql_group_stats", GC_STATS);
    return group_stats(g, {launches_update}, launches_sample, nullptr);
}
int fql_cfgrl_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample) {
    GROUP_ENTER(g, AgentKind::CFGRL, "fql_cfgrl_group_stats", GC_STATS);
    return group_stats(g, {launches_update}, launches_sample, nullptr);
}
int fql_sac_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample) {
    GROUP_ENTER(g, AgentKind::SAC, "fql_sac_group_stats", GC_STATS);
    return group_stats(g, {launches_update}, launches_sample, nullptr);
}

int fql_group_synchronize(fql_group g) {
    if (!g) { g_create_error = "fql_group_synchronize: NULL group"; return FQL_E_INVALID; }
    if ((g->last == hipStreamLegacy ? hipDeviceSynchronize() : hipEventSynchronize(g->ev_done)) != hipSuccess || hipStreamSynchronize(g->lanes[0]) != hipSuccess) {
        g_create_error = std::string("fql_group_synchronize: ") + hipGetErrorString(hipGetLastError());
        return FQL_E_HIP;
    }
    for (fql_handle h : g->m) h->grp_pending = false;
    return FQL_OK;
}

}  // extern "C"

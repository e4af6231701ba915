// Orchestration of the whole Allegro hot path behind the C ABI (include/allegro_amd.h):
// forward (allegro/model/allegro_models.py:222-297 module chain) and the hand-written reverse pass
// w.r.t. positions (what ForceStressOutput's autograd does, allegro_models.py:101-103).
// All kernels are enqueued on the caller's stream; all tensors live in caller-owned HBM buffers.
#include <algorithm>
#include <atomic>

#include "aa_common.h"

namespace aa {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int device_cu_count() {
  constexpr int kMaxDevices = 64;
  static std::atomic<int> cached[kMaxDevices];  // per device id, 0 = not asked yet
  int dev = 0, n = 0;
  AA_CHECK_HIP(hipGetDevice(&dev));
  const bool slot = dev >= 0 && dev < kMaxDevices;
  if (slot && (n = cached[dev].load(std::memory_order_relaxed)) > 0) return n;
  AA_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  if (n <= 0) return fail(AA_ERR_HIP, "hipDeviceGetAttribute: the device reports no compute units");
  if (slot) cached[dev].store(n, std::memory_order_relaxed);
  return n;
}
}  // namespace aa

using namespace aa;

// ------------------------------------------------------------------------------------------------
// TP operator plan (seam B1/B2)
// ------------------------------------------------------------------------------------------------
struct aa_tp_plan {
  aa_dtype dtype;
  TpLayerDev dev;
  std::vector<void*> owned;
  int spec_sig = -1;           // generated signature of this layer (aa_cg_gen.h) or -1
  bool dense_spec = false;     // forward / input gradients on the specialised dense-operand kernels (aa_tp_dense.hip)
};

extern "C" const char* aa_last_error(void) { return g_err.c_str(); }
extern "C" int aa_version(void) { return 1; }

extern "C" int aa_tp_plan_create(const aa_tp_desc* desc, aa_dtype dtype, aa_tp_plan** out) {
  AA_REQUIRE(desc && out, "aa_tp_plan_create: null argument");
  AA_REQUIRE(dtype == AA_F32 || dtype == AA_F64, "aa_tp_plan_create: bad dtype");
  aa_tp_plan* p = new aa_tp_plan();
  p->dtype = dtype;
  int rc = build_tp_layer(*desc, &p->dev, &p->owned);
  if (rc) {
    for (void* q : p->owned) (void)hipFree(q);
    delete p;
    return rc;
  }
  p->spec_sig = find_spec_sig(*desc);
  p->dense_spec = tp_dense_supported(p->spec_sig, desc->mul, dtype);
  *out = p;
  return AA_OK;
}

extern "C" int aa_tp_plan_use_general_kernels(aa_tp_plan* plan, int on) {
  AA_REQUIRE(plan, "aa_tp_plan_use_general_kernels: null plan");
  plan->dense_spec = !on && tp_dense_supported(plan->spec_sig, plan->dev.mul, plan->dtype);
  return AA_OK;
}

extern "C" int aa_tp_plan_is_specialised(const aa_tp_plan* plan) { return plan && plan->dense_spec ? 1 : 0; }

extern "C" void aa_tp_plan_destroy(aa_tp_plan* plan) {
  if (!plan) return;
  for (void* q : plan->owned) (void)hipFree(q);
  delete plan;
}

extern "C" int aa_tp_forward(const aa_tp_plan* plan, int64_t E, int64_t N, const void* x1, const void* x2,
                             const void* weights, const int32_t* rowptr, const int32_t* eids, double scatter_factor,
                             void* x2s, void* out, aa_stream stream) {
  AA_REQUIRE(plan && weights && rowptr && (N == 0 || x2s), "aa_tp_forward: null argument");
  AA_REQUIRE(E == 0 || (x1 && x2 && out), "aa_tp_forward: null edge tensor");
  if (E == 0) {  // a frame or shard without edges: no rows of x1 / x2 / out; the scatter-sum of nothing is zero
    const size_t row = size_t(plan->dev.mul) * plan->dev.d2 * (plan->dtype == AA_F32 ? 4 : 8);
    if (N > 0) AA_CHECK_HIP(hipMemsetAsync(x2s, 0, size_t(N) * row, static_cast<hipStream_t>(stream)));
    return AA_OK;
  }
  if (plan->dense_spec) {
    TpDenseArgs d{};
    d.E = E;
    d.N = N;
    d.rowptr = rowptr;
    d.eids = eids;
    d.u = plan->dev.mul;
    d.coupling = plan->dev.coupling;
    d.sf = scatter_factor;
    d.x1 = x1;
    d.x2 = x2;
    d.weights = weights;
    d.x2s = x2s;
    d.out = out;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return plan->dtype == AA_F32 ? launch_tp_dense<float>(plan->spec_sig, false, d, st) : launch_tp_dense<double>(plan->spec_sig, false, d, st);
  }
  TpLayerFwdArgs a{};
  a.E = E;
  a.N = N;
  a.rowptr = rowptr;
  a.eids = eids;
  a.x1.dense = x1;
  a.x2.dense = x2;
  a.weights = weights;
  a.scatter_factor = scatter_factor;
  a.x2s = x2s;
  a.out = out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return plan->dtype == AA_F32 ? launch_tp_layer_fwd<float>(plan->dev, a, s) : launch_tp_layer_fwd<double>(plan->dev, a, s);
}

extern "C" int aa_tp_backward(const aa_tp_plan* plan, int64_t E, int64_t N, const void* x1, const void* x2s,
                              const void* weights, const int32_t* rowptr, const int32_t* eids, double scatter_factor,
                              const void* gout, void* gx1, void* gx2, aa_stream stream) {
  AA_REQUIRE(plan && weights && rowptr, "aa_tp_backward: null argument");
  if (E == 0) return AA_OK;  // no edges: gx1 / gx2 have no rows, nothing is read or written
  AA_REQUIRE(gout && (gx1 || gx2), "aa_tp_backward: null argument");
  AA_REQUIRE((!gx1 || x2s) && (!gx2 || x1), "aa_tp_backward: a requested gradient's operand is null");
  if (plan->dense_spec) {
    TpDenseArgs d{};
    d.E = E;
    d.N = N;
    d.rowptr = rowptr;
    d.eids = eids;
    d.u = plan->dev.mul;
    d.coupling = plan->dev.coupling;
    d.sf = scatter_factor;
    d.x1 = x1;
    d.weights = weights;
    d.x2s = const_cast<void*>(x2s);
    d.gout = gout;
    d.gx1 = gx1;
    d.gx2 = gx2;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return plan->dtype == AA_F32 ? launch_tp_dense<float>(plan->spec_sig, true, d, st) : launch_tp_dense<double>(plan->spec_sig, true, d, st);
  }
  TpLayerBwdArgs a{};
  a.E = E;
  a.N = N;
  a.rowptr = rowptr;
  a.eids = eids;
  a.x1.dense = x1;
  a.weights = weights;
  a.scatter_factor = scatter_factor;
  a.x2s = x2s;
  a.gout = gout;
  a.g1.dense = gx1;
  a.g2.dense = gx2;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return plan->dtype == AA_F32 ? launch_tp_layer_bwd<float>(plan->dev, a, s) : launch_tp_layer_bwd<double>(plan->dev, a, s);
}

extern "C" int aa_tp_segment_sum(aa_dtype dtype, int64_t E, int64_t N, int64_t row_elems, const void* x, const int32_t* rowptr,
                                 const int32_t* eids, double scale, void* out, aa_stream stream) {
  AA_REQUIRE(rowptr && (N == 0 || row_elems == 0 || out) && (E == 0 || x), "aa_tp_segment_sum: null argument");
  AA_REQUIRE(dtype == AA_F32 || dtype == AA_F64, "aa_tp_segment_sum: dtype");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == AA_F32 ? launch_segment_sum<float>(N, row_elems, x, rowptr, eids, scale, out, s)
                         : launch_segment_sum<double>(N, row_elems, x, rowptr, eids, scale, out, s);
}

extern "C" size_t aa_tp_weights_workspace_bytes(const aa_tp_plan* plan, int64_t N) {
  if (!plan) return 0;
  const size_t elem = plan->dtype == AA_F32 ? 4 : 8;
  if (plan->dense_spec) return size_t(tp_wgrad_slots(N, kDenseWgradSlots) + 1) * plan->dev.mul * plan->dev.num_paths * elem;
  return tp_layer_wgrad_workspace_elems(plan->dev, N) * elem;
}

extern "C" int aa_tp_backward_weights(const aa_tp_plan* plan, int64_t E, int64_t N, const void* x1, const void* x2s,
                                      const int32_t* rowptr, const int32_t* eids, const void* gout, void* workspace,
                                      size_t workspace_bytes, void* gweights, aa_stream stream) {
  AA_REQUIRE(plan && rowptr && gweights, "aa_tp_backward_weights: null argument");
  AA_REQUIRE(E == 0 || (x1 && x2s && gout), "aa_tp_backward_weights: null tensor");
  AA_REQUIRE(workspace_bytes >= aa_tp_weights_workspace_bytes(plan, N) && (workspace || workspace_bytes == 0),
             "aa_tp_backward_weights: workspace too small");
  TpLayerWgradArgs a{};
  a.E = E;
  a.N = N;
  a.rowptr = rowptr;
  a.eids = eids;
  a.x1 = x1;
  a.x2s = x2s;
  a.gout = gout;
  a.partial = workspace;
  a.gw = gweights;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (plan->dense_spec)
    return plan->dtype == AA_F32 ? launch_tp_dense_wgrad<float>(plan->spec_sig, plan->dev.mul, plan->dev.coupling, a, s)
                                 : launch_tp_dense_wgrad<double>(plan->spec_sig, plan->dev.mul, plan->dev.coupling, a, s);
  return plan->dtype == AA_F32 ? launch_tp_layer_wgrad<float>(plan->dev, a, s) : launch_tp_layer_wgrad<double>(plan->dev, a, s);
}

// ------------------------------------------------------------------------------------------------
// model pipeline: which kernels a plan runs, decided once at plan time (choose_pipeline)
// ------------------------------------------------------------------------------------------------
// Tensor-product path, least to most specialised.  From Moments on the env weights go through per-atom moments: no [E,R*u]
// env tensors (TpMomArgs / TpOpArgs).
enum class TpPath {
  General,    // per-edge kernels on LDS coupling tables, reference layouts
  Spec,       // per-edge kernels with compile-time Clebsch-Gordan tables, channel-minor internal layouts
  SpecChain,  // ... with the 2-layer chain kernel for layer 1 (no [E,u,D] tensors in HBM)
  Moments,    // 2-layer moments kernels (u = 64)
  Operator,   // per-atom operator kernels (aa_tp_op.hip; any L <= 3, u = 64 m)
};
enum class LinearPath {
  Single,  // one launch per linear layer
  Slot,    // single layers on output-folded weights, reverse by dense-net slot (BlobLayout::s_*)
  Chains,  // MLP chains fused into gemm_chain_bf16x3_kernel (hidden layers stay in registers)
};

struct ModelPipeline {
  // widened sizes: the model's own where nothing was padded (aa_model_plan::u_raw / hid_raw keep those)
  int num_tensor, embed_width, latent_width, readout_width;
  int spec_sig[AA_MAX_LAYERS];  // generated-signature id per layer (at the widened channel count), or -1
  TpPath tp;
  int chain_pair;     // >= 0: pair id of a 2-layer stack on the chain kernels (SpecChain, Moments; an Operator plan keeps the id)
  int tp_op;          // >= 0: signature chain of the operator kernels (exactly the Operator plans)
  LinearPath linear;
  bool op_proj;       // Operator: the env projections as batched linear-layer launches (TpOpArgs::proj_gemm)
  bool two_body_table;       // blob carries [T*T][8][S0] type_embed(c | pair) * basis_linear[n][c] (spline models: the spline weights)
  bool embed_fused;          // reverse pass: d(two-body embedding) [E,S0] never materialised, the last reverse chain contracts it
                             // back to the 8 basis functions in its epilogue (embrev_out in aa_common.h)
  // weight folds the blob carries (aa_common.h; a fold that is off keeps its blob offsets at 0)
  bool fold_embed_table;     // the two-body table times the first scalar_embed_mlp layer
  bool fold_embed_output;    // W1 @ G0, W1 @ Wenv0: the output layer of scalar_embed_mlp folded into its consumers
  bool fold_latent_outputs;  // first layers of latent 1 / edge_readout / the readout-reverse chain with the latent output layers folded
  bool fold_lat0_reverse;    // ... and the chain's second layer with Wout_0^T folded into the lat0 columns (d a_0 instead of d lat0)
  bool fused_fwd;            // the whole forward as ONE per-atom-tile kernel when the graph allows (aa_fused.hip)
  bool fused_wide;           // ... its one-tile pass on the eight-wave form (two waves per SIMD, aa_fused8.hip)

  bool channel_minor() const { return tp != TpPath::General; }
  bool env_moments() const { return tp == TpPath::Moments || tp == TpPath::Operator; }
  bool chains() const { return linear == LinearPath::Chains; }  // (with them: the merged readout-reverse chain, o_b3{a,b,c}_q)
  bool slot() const { return linear == LinearPath::Slot; }
};

// The whole plan-time decision, from the caller's configuration and options alone: no HIP call, no allocation.
static ModelPipeline choose_pipeline(const aa_model_config& q, const aa_plan_options& opt) {
  const int L = q.num_layers, S = q.num_scalar, T = q.num_types, B = q.num_bessels, S0 = q.embed_dim;
  const bool f32 = q.dtype == AA_F32;
  // every fused fast path below has SiLU built in; the other nonlinearities run the general kernels
  const bool all_silu = q.act_kind[0] == AA_ACT_SILU && q.act_kind[1] == AA_ACT_SILU && q.act_kind[2] == AA_ACT_SILU;
  const bool scalars_ok = all_silu && (S == 64 || S == 128) && !opt.tp_no_moments;

  // ---- widened sizes ----
  // Channel padding.  A stack whose tensor-channel count is not a multiple of 64 (16 <= u < 256) is evaluated as the
  // next multiple-of-64 stack whose extra channels have zero weights: env_embed_linear / the env columns of first_proj and of the latent outputs / the scalar rows of
  // the latent inputs are zero-padded at pack time (aa_model_pack_weights), so the padded channels carry exact zeros
  // through every layer and the results are those of the narrow model -- which thereby runs the tuned 64-channel
  // kernels (moments or per-atom operator kernels, fused chains, fused forward) instead of the per-edge ones (BASELINE config 0, u = 32: 26 launches
  // and 0.40 ms per step on 64 atoms without, 15 launches with).  Only where the 64-channel stack takes that path: the
  // pad-eligible stack is the moments / operator shape below without the sizes that padding itself settles.
  const bool pad_stack = !opt.no_channel_padding && scalars_ok && (L == 2 || L == 3) && !opt.tp_generic && !opt.tp_no_chain;
  // Hidden-width padding, same idea: a single hidden layer narrower than 64 (the reference's constructor default for
  // edge_readout is 32, allegro_models.py:137) is zero-padded to 64 -- silu(0) = 0 and there are no biases, so the
  // extra units stay exactly zero -- which is what lets the stack run the fused linear-layer chains.
  auto widened = [&](int depth, int width) { return (pad_stack && depth == 1 && width >= 8 && width < 64) ? 64 : width; };
  const int He = widened(q.embed_mlp_depth, q.embed_mlp_width), H = widened(q.latent_mlp_depth, q.latent_mlp_width),
            Hr = widened(q.readout_mlp_depth, q.readout_mlp_width);
  const bool latents_ok = q.latent_mlp_depth >= 1 && (H == 64 || H == 128);
  const int u_pad = (q.num_tensor + 63) / 64 * 64;  // 16..63 -> 64 (moments / operator kernels), 65..127 -> 128, ... (operator kernels)
  const bool pad = pad_stack && latents_ok && q.num_tensor >= 16 && q.num_tensor != u_pad && u_pad <= 256;
  const int u = pad ? u_pad : q.num_tensor;
  const int Dsh = (q.l_max + 1) * (q.l_max + 1);

  // ---- shapes of the linear-layer paths ----
  const bool chains_shape = f32 && S == 64 && q.embed_mlp_depth == 1 && He == 64 && q.latent_mlp_depth == 1 && H == 64 &&
                            q.readout_mlp_depth == 1 && Hr == 64 && S0 % 32 == 0 && !opt.gemm_no_chain && !opt.gemm_fp32_mfma &&
                            !opt.gemm_valu;
  const bool slot_shape = !opt.no_slot_form && q.latent_mlp_depth == 1 && H == S && q.readout_mlp_depth >= 1 && q.embed_mlp_depth >= 1 &&
                          He == S && (Hr % 16) == 0;

  // ---- tensor-product path ----
  ModelPipeline m{};
  bool sigs_ok = !opt.tp_generic;
  for (int l = 0; l < L; ++l) {
    aa_tp_desc d = q.tps[l];
    if (pad) d.mul = u;
    m.spec_sig[l] = find_spec_sig(d);
    sigs_ok = sigs_ok && m.spec_sig[l] >= 0;
  }
  // fp64 at l_max=3 does not fit the register file (256 VGPR + 256 AGPR + 1.9 KB scratch per lane, and
  // wrong results on hardware in round 1): keep it on the general LDS-table kernels for now
  const bool spec = sigs_ok && !(q.dtype == AA_F64 && q.l_max >= 3);
  const int chain_pair = (spec && L == 2 && !opt.tp_no_chain) ? find_chain_pair(m.spec_sig[0], m.spec_sig[1]) : -1;
  // moments shape: a 2-layer chain pair at u = 64 whose workgroups (last term) fit the 160 KB of LDS
  const bool moments_ok = scalars_ok && latents_ok && chain_pair >= 0 && u == 64 &&
                          (f32 ? 4 : 8) * 4 * Dsh * (std::max(S, H) + 64 + 64) <= 160 * 1024;
  // operator shape: every standard stack the tuned 2-layer/u=64 kernels above do not cover (and, with
  // tp_force_operator, those too); they need the channel-minor layouts of the specialised path but none of its kernels,
  // so fp64 at l_max = 3 is fine here
  const bool operator_ok = scalars_ok && latents_ok && sigs_ok && L >= 2 && L <= 3 && (u % 64) == 0 && u <= 256 && !opt.tp_no_operator;
  // Where the 2-layer moments kernels apply but the fused chains do NOT (fp64; S or the MLP widths 128; deeper MLPs), the operator
  // kernels -- with the slot form of the linear layers where that applies -- are the faster pipeline: measured on the C3 box
  // (profiles/r05_v3_shape_map_c3.md against r05_v7 / r05_v8 with the operator path forced): fp32 u 64 / S 128 7.41 -> 3.96 ms,
  // fp64 u = S = 64 4.89 -> 4.14 ms, fp64 S 128 8.80 -> 6.82 ms; fp32 S 64 with 128-wide latents is a wash (3.70 vs 3.76 ms) and
  // keeps the moments kernels.
  const bool prefer_op = moments_ok && !chains_shape && (slot_shape || !f32) && !opt.tp_prefer_moments;
  const int tp_op = (operator_ok && (!moments_ok || opt.tp_force_operator || prefer_op)) ? find_op_chain(m.spec_sig, L) : -1;
  m.tp = tp_op >= 0 ? TpPath::Operator : moments_ok ? TpPath::Moments : chain_pair >= 0 ? TpPath::SpecChain : spec ? TpPath::Spec : TpPath::General;
  m.chain_pair = chain_pair;
  m.tp_op = tp_op;
  m.op_proj = tp_op >= 0 && opt.op_proj_gemm != 2;

  // ---- linear-layer path, folds ----
  const bool chains = m.env_moments() && (tp_op < 0 || u == 64) && chains_shape;
  m.linear = chains ? LinearPath::Chains : (tp_op >= 0 && slot_shape) ? LinearPath::Slot : LinearPath::Single;
  // two-body table [T*T][B][S0] (type embedding x basis weights): the last reverse chain contracts against it (<= 2
  // species: its LDS copy must leave room for three workgroups per CU) and the fused forward evaluates the embedding
  // from it (<= 3 species: 18 KB of its LDS).  Part of the blob whenever the shapes allow -- not a function of the options.
  const bool tab_ok = chains && T <= 3 && B == 8 && S0 == 64;
  m.two_body_table = tab_ok || q.embed_kind == 1;
  m.embed_fused = tab_ok && T <= 2 && !opt.embed_no_fuse;
  m.fold_embed_table = tab_ok;  // (the fold needs a hidden layer of 64 behind the embedding: what the chains have)
  const bool chains2 = chains && L == 2;  // (chains: u = 64, S = every MLP width = 64, one hidden layer each)
  m.fold_embed_output = chains2;
  m.fold_latent_outputs = chains2;
  m.fold_lat0_reverse = chains2;

  // ---- fused forward ----
  // fused per-atom-tile forward (aa_fused.hip): the standard 2-layer 64-wide fp32 stack with the
  // two-body table in LDS; same parity tests as the staged pipeline.  With the tensor-track scalars accumulated in
  // anchored program order (aa::anchor -- the kernel used to carry 70-350 spilled VGPRs) the 32-edge-tile form beats the
  // staged forward at every size on MI355X: 22-24 % of the step on 64-1000 atoms (one launch instead of seven), 9 % at
  // 4096, 4.5 % at 10 648, 0.5 % at 97 336 atoms, and it moves 2.1 instead of 7.3 KB/edge (profiles/archive/r02_v23_fused_sweep.log).
  // aa_plan_options.fused_forward: 0 / 1 = whenever the graph allows (automatic), 3 = never (staged pipeline); A/B: 2 = also for every
  // graph with segments <= 128, in the pure team form, 4 = the same in the mixed form.
  // Eligible: the moments kernels of l_max 1 / 2 with every fold of the kernel's weight program packed.
  const bool fused = m.tp == TpPath::Moments && (chain_pair == 0 || chain_pair == 1) && m.fold_embed_table && m.fold_embed_output &&
                     m.fold_latent_outputs && opt.fused_forward != 3;
  m.fused_fwd = fused;
  // the two-waves-per-SIMD form (aa_fused8.hip) needs a two-body table that leaves 16.6 KB of LDS per wave (one species)
  m.fused_wide = fused && opt.fused_narrow != 1 && fused_fwd8_lds_bytes(T, 8) <= 160 * 1024;
  m.num_tensor = u;
  m.embed_width = He;
  m.latent_width = H;
  m.readout_width = Hr;
  return m;
}

// ------------------------------------------------------------------------------------------------
// step plan: which launches ONE step consists of, decided once per step (choose_step)
// ------------------------------------------------------------------------------------------------
// What the plan cannot say, because it also depends on the graph of this step, on whether forces were asked for, on the debug
// taps and on the device.  run_model fills StepInputs from its arguments, choose_step turns them into one StepPlan, and Runner
// only reads that value: the forward and the reverse pass cannot disagree about what the other one did.
struct StepInputs {
  bool f32;                 // dtype of the plan
  bool taps;                // aa_model_plan_enable_taps: every tap is materialised
  bool with_forces;
  bool transposed_csr;      // aa_graph::t_rowptr / t_perm are present
  int64_t atoms, edges;     // of the graph
  int64_t atom0, atom_end;  // the active block: the atom-block hint, or every atom
  int64_t max_degree;       // aa_graph::max_degree, 0 = unknown
  bool pair_zbl;            // aa_model_plan_set_pair_zbl: the plan carries a ZBL pair potential
  bool block;               // internal, off for every public single-step entry point: the step is one block of a blocked step
                            // (aa_model_energy_forces_blocked)
};

enum class ForwardKind {
  Staged,        // one launch per stage
  StagedFolded,  // ... with the chains in the folded form of the fused forward (a_e / a_0 stored where the embedding / lat_0 used to be)
  FusedOneTile,  // ONE kernel, every segment in one 32-edge tile (aa_fused.hip / aa_fused8.hip)
  FusedTeam,     // ONE kernel, teams of 1 / 2 / 4 waves per atom for every atom
  FusedMixed,    // one-tile pass over all atoms (the long ones skipped) + team pass over the long ones
};
// Reverse stages the forward of this step already ran, as a depth (the values are the `tail` of fused_fwd8_num_steps)
enum class ReverseInForward {
  None = 0,
  Chain = 1,                // the readout-reverse chain (FusedForm::EightWaveTail)
  ChainMomentsLatent0 = 2,  // ... and behind it the layer-1 moments reverse and the latent-0 reverse chain (FusedForm::EightWaveDeepTail)
};
// Form of the reverse of the latent MLPs below the last one (the last one's rides in the readout-reverse chain where there are chains)
enum class LatentReverse {
  Mlp,            // mlp_bwd: one launch per layer (every plan without the chains)
  TwoLayerChain,  // output layer + first layer in one chain kernel
  FoldedChain,    // fold_lat0_reverse: ONE layer behind the operand transform, general chain kernel
  Resident,       // ... with its weights resident in LDS (aa_chain_res.hip)
  InForwardTail,  // ran in the deep tail of the fused forward
};

struct StepPlan {
  ForwardKind forward;
  FusedForm fused_form;                 // fused forwards: form of the one-tile pass (OneWave where there is none)
  bool slot;                            // slot form of the single-layer pipeline (LinearPath::Slot): forward stages and backward_slot
  bool op_split;                        // operator kernels: per-atom vectors through HBM, edge loops in lean kernels (off: tp_operator_fused)
  bool op_split_reverse;                // ... the moment gradients of the reverse too (a force step's workspace holds them)
  bool proj_forward, proj_reverse;      // operator kernels: the env projections as batched linear-layer launches (ModelPipeline::op_proj)
  bool readout_grad_in_reduce;          // readout_reduce also writes d E / d (last readout hidden layer): no readout_backward launch
  ReverseInForward reverse_in_forward;  // the reverse pass launches none of these
  LatentReverse latent_reverse;
  bool gather;                          // deterministic force assembly over the transposed CSR (off: atomics)
  bool zero_gsh, zero_forces;           // the reverse pass accumulates into d Y / the forces: zeroed first
  bool pair_zbl;                        // ZBL pair potential: one launch behind the forward (energy only) or in edge_tail (force step)
  bool mom0_in_chain;                   // layer-0 moments reverse: tp_mom_bwd_first stops after GM0 and the last reverse chain applies it to its own
                                        // rows in its epilogue (d a_e never stored, the layer-0 slab of d Y written there)
  bool block;                           // one block of a blocked step (the ONE place that says so; Runner reads it): only the block's atoms get their
                                        // energy written; with forces dvec / vec rows go to the frame-wide arrays in the gather form (no atomics) and the
                                        // caller assembles the forces

  bool fused() const { return forward == ForwardKind::FusedOneTile || forward == ForwardKind::FusedTeam || forward == ForwardKind::FusedMixed; }
  // did the forward of this step leave a_e in the embedding's slot (folded first stage / env weights in the reverse)?
  bool folded_first_stage() const { return forward != ForwardKind::Staged; }
};

static ReverseInForward fused_tail(FusedForm form) {
  return form == FusedForm::EightWaveDeepTail ? ReverseInForward::ChainMomentsLatent0
         : form == FusedForm::EightWaveTail   ? ReverseInForward::Chain
                                              : ReverseInForward::None;
}

static ForwardKind choose_forward(const ModelPipeline& pipe, const aa_plan_options& opt, const aa_model_config& c, const StepInputs& in) {
  // the staged forward chains in the same folded form as the fused forward (fold_embed_output, fold_latent_outputs): the hidden activations a_e /
  // a_0 are stored where the embedding / lat_0 used to be (ChainLayer::kept_out), consumers run on the folded matrices.  What
  // graphs with long segments -- dense systems, too large for the team form -- run.
  const bool fold_staged = pipe.chains() && pipe.tp_op < 0 && pipe.fold_embed_output && pipe.fold_latent_outputs && c.num_layers == 2 && !in.taps &&
                           !opt.staged_no_fold;
  const ForwardKind staged = fold_staged ? ForwardKind::StagedFolded : ForwardKind::Staged;
  // the whole forward in one launch (aa_fused.hip): every center atom's edge segment fits one 32-row MFMA tile
  if (!(in.f32 && pipe.fused_fwd && !in.taps && in.max_degree > 0 && in.max_degree <= kFusedMaxDegree)) return staged;
  const bool long_segments = in.max_degree > 32;
  // (three species + the team exchange area exceed the 160 KB of LDS: such graphs run the staged pipeline)
  if (fused_fwd_lds_bytes(c.num_types, long_segments) > size_t(160) * 1024) return staged;
  if (!long_segments) return ForwardKind::FusedOneTile;  // one full-ish tile per atom: faster than the staged forward at every size
  // Team form (2 / 4 tiles per atom): a tile costs the same whether 32 or 12 of its rows carry an edge, so it pays where
  // the step is latency-bound (few tiles: one launch instead of seven) or the tiles are nearly full.  Measured on Si boxes
  // at r_max 6 / 7 (44 / 73 edges per atom, profiles/archive/r03_p_*): 216-512 atoms 17-27 % faster than the staged step, 1 728
  // atoms -2 % / +8 %, 10 648 atoms +10 % / +18 % slower (69 % / 57 % of the tile rows in use).
  // (in.edges IS the edge count of the active block: the atom-block hint promises that every center with edges lies in
  // [atom_begin, atom_end) -- verified on the device by graph_hint_check_kernel -- so rowptr[atom_end] - rowptr[atom_begin],
  // which the host does not hold, equals aa_graph::num_edges)
  const int64_t n_active = in.atom_end - in.atom0;
  const int64_t tiles = n_active * (in.max_degree <= 64 ? 2 : 4);  // (upper bound: every atom at the class of the longest segment)
  const double fill = double(in.edges) / (32.0 * double(std::max<int64_t>(n_active, 1)));
  const bool avg_fits_one_tile = fill <= 1.15;
  // mixed form (one-tile pass over all atoms + team pass over the long ones) where long atoms are the minority -- boxes whose
  // average atom fits one tile; dense boxes that took the team path because they are small or their tiles are full run the pure
  // team form: there the one-tile launch would only skip.  2 / 4: the team / mixed form for every graph (A/B)
  const ForwardKind team = opt.fused_forward == 2 ? ForwardKind::FusedTeam
                           : (opt.fused_forward == 4 || avg_fits_one_tile) ? ForwardKind::FusedMixed
                                                                           : ForwardKind::FusedTeam;
  if (opt.fused_forward == 2 || opt.fused_forward == 4) return team;  // (A/B: the team / mixed form whenever segments fit it)
  // Round 5: a box whose AVERAGE atom fills most of one tile but whose longest segment is a little over 32 (thermal disorder: a
  // handful of Si atoms with 33..37 neighbours after 50 fs at 300 K) takes the MIXED form -- one-tile kernel over all atoms, the
  // team kernel over the long ones only (launch_fused_fwd) -- instead of giving up the fused forward for the whole box
  // (tools/md_loop.py at C4: staged 11.3 ms, team form for every atom 12.2 ms per step; profiles/r05_v2*_md_loop_*).
  if (fill >= 0.6 && avg_fits_one_tile) return team;
  return (tiles <= kFusedTeamTilesSmall || double(in.edges) >= 0.85 * 32.0 * double(tiles)) ? team : staged;
}

// The two-waves-per-SIMD forms (aa_fused8.hip) need a plan with fused_wide and a one-tile pass (no class lists, or the mixed
// form); they are the forms whose choice reads the CU count
static bool wide_one_tile_pass(const ModelPipeline& pipe, ForwardKind forward) {
  return pipe.fused_wide && (forward == ForwardKind::FusedOneTile || forward == ForwardKind::FusedMixed);
}

// The whole per-step decision, from the plan (`pipe`, `opt`, `c`: the configuration at the widened sizes), the step's inputs and
// the CU count of the device (read only where wide_one_tile_pass says so) alone: no HIP call, no allocation.
constexpr int64_t kMom0EpilogueEdges = int64_t(256) * 3 * 128;  // (see StepPlan::mom0_in_chain in choose_step)
static StepPlan choose_step(const ModelPipeline& pipe, const aa_plan_options& opt, const aa_model_config& c, const StepInputs& in, int cus) {
  const int64_t n = in.atom_end - in.atom0;
  const bool two_layer_chains = pipe.chains() && c.num_layers == 2;
  StepPlan s{};
  s.forward = choose_forward(pipe, opt, c, in);

  // ---- form of the one-tile pass of the fused forward (FusedForm), decided here only.  aa_plan_options.fused_narrow:
  //  0: boxes that leave a CU at most one workgroup (n <= 4 per CU) run one wave per SIMD whatever the kernel: there the
  //     register-rich one-wave form -- w0 held, operands kept split -- is the faster one (64 atoms 44 vs 48 us, profiles/r06_v4_ab_c2_*).
  //     From kFusedTailAtomsPerCu atoms per CU on, eight waves with the readout-reverse chain of the reverse pass in the tail, where
  //     that applies (forces requested, no team pass -- its atoms would miss it -- and the chain's folded weights): there the eight-wave
  //     form is as fast as two four-wave workgroups and the chain's 0.75 ms of streaming disappear (C4 -0.45 ms same box,
  //     profiles/r06_v19_*).  Otherwise two four-wave workgroups per CU.
  //     Where the resident latent-0 chain would run behind it (fold_lat0_reverse, fp32, S = u = latent width = 64) the tail is the DEEP
  //     one: the layer-1 moments reverse and that chain run in it too, and the reverse pass skips both launches (reverse_in_forward).
  //  2: eight waves at any size, with the (deep) tail where it applies;  3: four waves at any size, no tail;  1: never (fused_wide is off);
  //  4: eight waves at any size with the chain-only tail where a tail applies (A/B of the deep tail).
  const bool resident_shape = in.f32 && c.num_scalar == 64 && c.num_tensor == 64;  // (what aa_chain_res.hip and the deep tail are written for)
  const bool tail_ok = in.with_forces && s.forward == ForwardKind::FusedOneTile && two_layer_chains && pipe.fold_latent_outputs;
  const bool deep_ok = tail_ok && pipe.fold_lat0_reverse && pipe.env_moments() && resident_shape && c.latent_mlp_width == 64 && opt.fused_narrow != 4;
  const FusedForm tail_form = deep_ok ? FusedForm::EightWaveDeepTail : FusedForm::EightWaveTail;
  s.fused_form = !wide_one_tile_pass(pipe, s.forward)                ? FusedForm::OneWave
                 : (opt.fused_narrow == 2 || opt.fused_narrow == 4) ? (tail_ok ? tail_form : FusedForm::EightWave)
                 : opt.fused_narrow == 3                             ? FusedForm::FourWave
                 : n <= int64_t(4) * cus                             ? FusedForm::OneWave
                 : (tail_ok && n >= int64_t(kFusedTailAtomsPerCu) * cus) ? tail_form
                                                                         : FusedForm::FourWave;
  s.reverse_in_forward = n > 0 ? fused_tail(s.fused_form) : ReverseInForward::None;  // (an empty block launches nothing)

  // ---- linear layers ----
  // slot form of the single-layer pipeline (LinearPath::Slot); the debug taps name tensors it never forms
  s.slot = pipe.slot() && !in.taps;
  s.readout_grad_in_reduce = in.with_forces && !pipe.chains() && c.readout_mlp_depth > 0 && !opt.readout_two_pass;
  s.latent_reverse = !pipe.chains()                                                     ? LatentReverse::Mlp
                     : s.reverse_in_forward == ReverseInForward::ChainMomentsLatent0 ? LatentReverse::InForwardTail
                     : !(pipe.fold_lat0_reverse && c.num_layers == 2)                ? LatentReverse::TwoLayerChain
                     : (resident_shape && !opt.chain_staged_weights)                 ? LatentReverse::Resident
                                                                                     : LatentReverse::FoldedChain;

  // ---- layer-0 moments reverse: its per-edge half in the epilogue of the last reverse chain ----
  // Where the folded one-layer last chain with the embedding contraction runs behind the moments kernels (fp32, l_max <= 2: what the chain's
  // epilogue is compiled for).  aa_plan_options.mom0_epilogue: 0 = from kMom0EpilogueEdges edges on, 1 = wherever it applies, 2 = never.
  // The threshold is one resident round of the chain on the chip (256 CUs x 3 workgroups x 128 rows): what the form saves is HBM traffic,
  // and a step with fewer rows than that is bound by launch latency, not by traffic.
  const bool mom0_ok = in.with_forces && in.f32 && s.folded_first_stage() && pipe.tp == TpPath::Moments && pipe.chains() && pipe.embed_fused &&
                       pipe.fold_embed_table && (pipe.chain_pair == 0 || pipe.chain_pair == 1) && c.num_scalar == 64;
  s.mom0_in_chain = mom0_ok && opt.mom0_epilogue != 2 && (opt.mom0_epilogue == 1 || in.edges >= kMom0EpilogueEdges);

  // ---- operator kernels ----
  // split form (default): per-atom vectors through HBM, edge loops in lean kernels (tp_operator_fused: fused form)
  s.op_split = pipe.tp_op >= 0 && !opt.tp_operator_fused;
  s.op_split_reverse = s.op_split && in.with_forces;
  // env projections of the operator kernels as batched linear-layer launches (ModelPipeline::op_proj): where there are enough
  // atoms to fill the chip with 128-row tiles
  s.proj_forward = pipe.op_proj && s.op_split && (opt.op_proj_gemm == 1 || n >= 4096);
  s.proj_reverse = s.proj_forward && in.with_forces;

  // ---- what the reverse pass sums into ----
  s.block = in.block;
  s.gather = in.transposed_csr || (s.block && in.with_forces);
  // spec path with u <= 64 writes every g_sh slot with plain stores; otherwise slots are accumulated into
  s.zero_gsh = in.with_forces && !((pipe.channel_minor() && c.num_tensor <= 64) || pipe.tp_op >= 0);
  s.zero_forces = in.with_forces && !s.gather;
  s.pair_zbl = in.pair_zbl;
  return s;
}

// ------------------------------------------------------------------------------------------------
// model plan
// ------------------------------------------------------------------------------------------------
struct MlpLayout {
  std::vector<int> dims;        // d_0 .. d_n
  std::vector<size_t> w, wt;    // blob offsets (elements) of W_i [d_i,d_{i+1}] and its transpose
  std::vector<size_t> wp, wtp;  // the same two matrices in MFMA fragment order (aa_gemm.hip v3)
  std::vector<size_t> wq, wtq;  // ... and split into 3 bf16 levels (bf16x3 path; fp32 plans only)
};

// one linear layer's matrix in the three forms the single-layer kernels take (row-major, MFMA fragment order, bf16x3 levels)
struct GemmMat {
  size_t w = 0, wp = 0, wq = 0;
  int K = 0, N = 0;
};

// a set of equally shaped matrices at uniform strides (GemmArgs::batch)
struct GemmMatSet {
  size_t w = 0, wp = 0, wq = 0, w_bs = 0, wp_bs = 0, wq_bs = 0;
  int K = 0, N = 0, count = 0;
};

static std::vector<int> mlp_dims(int in, int depth, int width, int out) {
  std::vector<int> d{in};
  for (int i = 0; i < depth; ++i) d.push_back(width);
  d.push_back(out);
  return d;
}

// Where every entry of the packed weight blob lies (element offsets) and what shape it has.  layout_blob is the only writer: the
// plan keeps the value, and the packer, the Runner, layout_workspace and the debug taps read it.
struct BlobLayout {
  size_t o_rmax = 0, o_bessel = 0, o_cemb = 0, o_nemb = 0, o_basis = 0, o_g0 = 0, o_g0t = 0, o_g0p = 0, o_g0tp = 0, o_g0q = 0, o_g0tq = 0,
         o_b3a_q = 0, o_b3b_q = 0, o_b3c_q = 0, o_ro_last = 0, o_scales = 0, o_shifts = 0, n_elems = 0;
  size_t o_tpw[AA_MAX_LAYERS] = {};
  MlpLayout embed, readout;          // readout: only the GEMM layers (all but the final ->1 layer)
  MlpLayout latent[AA_MAX_LAYERS];
  int ro_last_dim = 0;               // input dim of the final readout linear
  // the optional parts: positions only, 0 where the part is absent -- whether it exists is the pipeline's to say
  size_t o_embtab = 0;               // (two_body_table) [T*T][8][64] type_embed(c | pair) * basis_linear[n][c]
  size_t o_embtab_h = 0;             // (fold_embed_table) [T*T][8][64] the same table times the first scalar_embed_mlp layer
  size_t o_lat1in_fq = 0, o_ro0_fq = 0;  // (fold_latent_outputs, 2-layer 64-wide stacks) bf16x3 copies of the first layers of latent 1 / edge_readout with the
                                     // latent output layers folded into their lat_l row blocks
  size_t o_b3af_q = 0;               // ... and of the merged first layer of the readout-reverse chain
  size_t o_b3bf_q = 0;               // (fold_lat0_reverse) ... and of its second layer with Wout_0^T folded into the lat0 columns (d a_0 instead of d lat0)
  size_t o_g0fq = 0, o_g0tfq = 0;    // (fold_embed_output) bf16x3 copies of W1 @ G0 [64, ng0] and of its transpose
  size_t o_wk0f = 0, o_wt0f = 0;     // (fold_embed_output) W1 @ Wenv0 as [k][R][u] and [R][u][k]
  // "Slot form" of the single-layer pipeline (LinearPath::Slot; operator-kernel plans: C5 and every standard stack off the tuned 2-layer shape).
  // The same algebra as fold_embed_output / fold_latent_outputs (aa_common.h), for any depth: the output layer of scalar_embed_mlp and of every latent MLP is
  // folded into its consumers at pack time, so slot l + 1 of the dense-net buffer holds the latent's hidden PRE-ACTIVATION z_l
  // (consumers activate those columns on load, GemmArgs::act_lo / act_hi) and the layers "a -> lat_l" do not exist.  The reverse
  // is evaluated BY SLOT, not by consumer: d z_l = ([d readout hidden | d z_{l+1} .. d z_{L-1}] @ stack_l + d a_l of the moments)
  // * act'(z_l) -- one K-stacked layer with 128-wide output per latent (the accumulator-resident kernel's shape, every slot
  // written once) instead of wide accumulate-into-the-dense-net layers.
  GemmMat s_g0f, s_g0ft;             //   W_last(embed) @ G0 [He, ng0] and its transpose
  GemmMat s_in[AA_MAX_LAYERS];       //   first layer of latent l with the row blocks of earlier latents folded  [S (l+1) + u, H]
  GemmMat s_ro0;                     //   first readout layer, folded                                             [SL1, Hr]
  GemmMat s_rs[AA_MAX_LAYERS];       //   reverse stack of slot l + 1: rows [readout | latent l+1 .. L-1] -> d a_l  [Hr + S (L-1-l), H]
  GemmMat s_rstb;                    //   reverse stack of slot 0 (two-body): rows [readout | latent 0 .. L-1]      [Hr + S L, S]
  GemmMat s_sct[AA_MAX_LAYERS];      //   d z_l -> d (tensor scalars of layer l)                                   [H, u]
  size_t o_s_wk0 = 0, o_s_wt0 = 0;   //   W_last(embed) @ Wenv0 as [k][R][u] and [R][u][k]
  // operator-kernel plans (pipe.op_proj): the env projections as batched linear-layer launches (TpOpArgs::proj_gemm) -- per layer the R matrices
  // f Wenv_l[:, r, :] [ka, u] and their transposes [u, ka]; layer 0 also behind the output layer of scalar_embed_mlp (slot form)
  GemmMatSet s_pr[AA_MAX_LAYERS], s_prt[AA_MAX_LAYERS], s_pr0f, s_prt0f;
  int ng0 = 0;                       // output width of the fused first-stage GEMM
  size_t o_wk[AA_MAX_LAYERS] = {}, o_wt[AA_MAX_LAYERS] = {};  // (moments / operator plans) Wenv of layer l as [ka][R][u] and [R][u][ka]

  uint64_t hash(const aa_model_config& c, const ModelPipeline& pipe, int u_raw) const;
};

// The blob layout of a pipeline, from the widened configuration and the pipeline alone: no HIP call, nothing read from a plan.
// THE ORDER OF THE take() CALLS IS THE BLOB FORMAT: every entry starts on a multiple of 64 elements, in the order taken.
static BlobLayout layout_blob(const aa_model_config& c, const ModelPipeline& pipe) {
  BlobLayout b;
  const int L = c.num_layers, S = c.num_scalar, u = c.num_tensor, T = c.num_types, B = c.num_bessels, S0 = c.embed_dim;
  const int R = c.l_max + 1, W = R * u, SL1 = S * (L + 1), Hr = c.readout_mlp_width, H = c.latent_mlp_width;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += (n + 63) / 64 * 64;
    return r;
  };
  auto lay = [&](MlpLayout& m, const std::vector<int>& dims, int nlayers) {
    m.dims = dims;
    for (int i = 0; i < nlayers; ++i) {
      m.w.push_back(take(size_t(dims[i]) * dims[i + 1]));
      m.wt.push_back(take(size_t(dims[i]) * dims[i + 1]));
      m.wp.push_back(take(gemm_packed_elems(dims[i], dims[i + 1])));
      m.wtp.push_back(take(gemm_packed_elems(dims[i + 1], dims[i])));
      m.wq.push_back(take(gemm_bf16x3_words(dims[i], dims[i + 1])));
      m.wtq.push_back(take(gemm_bf16x3_words(dims[i + 1], dims[i])));
    }
  };
  // (braced initialisers are evaluated left to right: w, wp, wq are taken in this order)
  auto mat = [&](int K, int N) { return GemmMat{take(size_t(K) * N), take(gemm_packed_elems(K, N)), take(gemm_bf16x3_words(K, N)), K, N}; };
  auto mset = [&](int K, int N, int count) {
    auto r64 = [](size_t n) { return (n + 63) / 64 * 64; };
    const size_t w_bs = r64(size_t(K) * N), wp_bs = r64(gemm_packed_elems(K, N)), wq_bs = r64(gemm_bf16x3_words(K, N));
    return GemmMatSet{take(w_bs * count), take(wp_bs * count), take(wq_bs * count), w_bs, wp_bs, wq_bs, K, N, count};
  };
  b.o_rmax = take(size_t(T) * T);
  b.o_bessel = take(B);
  b.o_cemb = take(size_t(T) * S0 / 2);
  b.o_nemb = take(size_t(T) * S0 / 2);
  b.o_basis = take(size_t(B) * S0);
  lay(b.embed, mlp_dims(S0, c.embed_mlp_depth, c.embed_mlp_width, S), c.embed_mlp_depth + 1);
  b.ng0 = pipe.env_moments() ? S + W : S + 2 * W;
  b.o_g0 = take(size_t(S) * b.ng0);
  b.o_g0t = take(size_t(S) * b.ng0);
  b.o_g0p = take(gemm_packed_elems(S, b.ng0));
  b.o_g0tp = take(gemm_packed_elems(b.ng0, S));
  b.o_g0q = take(gemm_bf16x3_words(S, b.ng0));
  b.o_g0tq = take(gemm_bf16x3_words(b.ng0, S));
  if (pipe.env_moments()) {
    for (int l = 0; l < L; ++l) {
      const size_t ka = l == 0 ? S : H;
      b.o_wk[l] = take(ka * W);
      b.o_wt[l] = take(ka * W);
    }
  }
  for (int l = 0; l < L; ++l) {
    int in = S * (l + 1) + u, outd = S + ((l < L - 1 && !pipe.env_moments()) ? W : 0);
    lay(b.latent[l], mlp_dims(in, c.latent_mlp_depth, H, outd), c.latent_mlp_depth + 1);
    b.o_tpw[l] = take(size_t(c.tps[l].coupling ? u : 1) * c.tps[l].num_paths);
  }
  {
    std::vector<int> rd = mlp_dims(SL1, c.readout_mlp_depth, Hr, 1);
    lay(b.readout, rd, c.readout_mlp_depth);  // all but the last layer
    b.ro_last_dim = rd[rd.size() - 2];
    b.o_ro_last = take(b.ro_last_dim);
  }
  if (pipe.fold_embed_output) {
    b.o_g0fq = take(gemm_bf16x3_words(64, b.ng0));
    b.o_g0tfq = take(gemm_bf16x3_words(b.ng0, 64));
    b.o_wk0f = take(size_t(64) * W);
    b.o_wt0f = take(size_t(64) * W);
  }
  if (pipe.fold_latent_outputs) {  // (S = u = every MLP width = 64, one hidden layer each, L = 2)
    b.o_lat1in_fq = take(gemm_bf16x3_words(2 * S + u, 64));
    b.o_ro0_fq = take(gemm_bf16x3_words(3 * S, 64));
    b.o_b3af_q = take(gemm_bf16x3_words(64, 64));
    b.o_b3bf_q = pipe.fold_lat0_reverse ? take(gemm_bf16x3_words(128, S * L)) : 0;
  }
  b.o_embtab = pipe.two_body_table ? take(size_t(T) * T * B * S0) : 0;
  b.o_embtab_h = pipe.fold_embed_table ? take(size_t(T) * T * B * 64) : 0;
  if (pipe.chains()) {
    // merged reverse chain "readout' o latent_{L-1}'" (see Runner::backward): the readout-reverse columns that feed
    // the last latent, and [readout-reverse columns of the earlier features (zero-padded) ; latent-reverse] stacked
    b.o_b3a_q = take(gemm_bf16x3_words(64, S));
    b.o_b3b_q = take(gemm_bf16x3_words(128, S * L));
    b.o_b3c_q = take(gemm_bf16x3_words(64, u));
  }
  if (pipe.slot()) {
    b.s_g0f = mat(S, b.ng0);
    b.s_g0ft = mat(b.ng0, S);
    for (int l = 0; l < L; ++l) {
      b.s_in[l] = mat(S * (l + 1) + u, H);
      b.s_rs[l] = mat(Hr + S * (L - 1 - l), H);
      b.s_sct[l] = mat(H, u);
    }
    b.s_ro0 = mat(SL1, Hr);
    b.s_rstb = mat(Hr + S * L, S);
    b.o_s_wk0 = take(size_t(S) * W);
    b.o_s_wt0 = take(size_t(S) * W);
  }
  if (pipe.op_proj) {
    for (int l = 0; l < L; ++l) {
      const int ka = l == 0 ? S : H;
      b.s_pr[l] = mset(ka, u, R);
      b.s_prt[l] = mset(u, ka, R);
    }
    if (pipe.slot()) {
      b.s_pr0f = mset(S, u, R);
      b.s_prt0f = mset(u, S, R);
    }
  }
  b.o_scales = take(T);
  b.o_shifts = take(T);
  b.n_elems = o;
  return b;
}

// FNV-1a over every quantity the blob is laid out by (aa_model_plan_layout_hash: exported packages and host model files carry
// the value, so neither the quantities nor their order may change).  The lists below are kept by hand, and still no new entry
// can go unnoticed: n_elems and the offset of every later entry -- o_scales and o_shifts at least -- move when one is added.
uint64_t BlobLayout::hash(const aa_model_config& c, const ModelPipeline& pipe, int u_raw) const {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (v >> (8 * i)) & 0xff;
      h *= 1099511628211ull;
    }
  };
  auto mixv = [&](const std::vector<size_t>& v) {
    mix(v.size());
    for (size_t x : v) mix(x);
  };
  auto mixm = [&](const MlpLayout& m) {
    mix(m.dims.size());
    for (int d : m.dims) mix(uint64_t(d));
    mixv(m.w); mixv(m.wt); mixv(m.wp); mixv(m.wtp); mixv(m.wq); mixv(m.wtq);
  };
  for (uint64_t v : {uint64_t(c.dtype), uint64_t(c.num_types), uint64_t(c.num_bessels), uint64_t(c.l_max), uint64_t(c.num_layers),
                     uint64_t(c.num_scalar), uint64_t(c.num_tensor), uint64_t(c.embed_dim), uint64_t(c.embed_mlp_width),
                     uint64_t(c.latent_mlp_width), uint64_t(c.readout_mlp_width), uint64_t(u_raw), uint64_t(pipe.channel_minor()),
                     uint64_t(pipe.env_moments()), uint64_t(pipe.chains()), uint64_t(pipe.chain_pair + 1), uint64_t(pipe.tp_op + 1), uint64_t(ng0),
                     uint64_t(n_elems), uint64_t(pipe.slot())})
    mix(v);
  if (pipe.slot()) {
    auto mixg = [&](const GemmMat& m) { mix(m.w); mix(m.wp); mix(m.wq); };
    mixg(s_g0f); mixg(s_g0ft); mixg(s_ro0); mixg(s_rstb);
    for (int l = 0; l < c.num_layers; ++l) { mixg(s_in[l]); mixg(s_rs[l]); mixg(s_sct[l]); }
    mix(o_s_wk0); mix(o_s_wt0);
  }
  if (pipe.op_proj) {
    auto mixs = [&](const GemmMatSet& m) { mix(m.w); mix(m.wp); mix(m.wq); mix(m.w_bs); };
    for (int l = 0; l < c.num_layers; ++l) { mixs(s_pr[l]); mixs(s_prt[l]); }
    mixs(s_pr0f); mixs(s_prt0f);
  }
  for (size_t v : {o_rmax, o_bessel, o_cemb, o_nemb, o_basis, o_g0, o_g0t, o_g0p, o_g0tp, o_g0q, o_g0tq,
                   o_b3a_q, o_b3b_q, o_b3c_q, o_ro_last, o_scales, o_shifts, o_embtab, o_embtab_h, o_lat1in_fq, o_ro0_fq, o_b3af_q, o_b3bf_q, o_g0fq, o_g0tfq, o_wk0f, o_wt0f})
    mix(v);
  for (int l = 0; l < c.num_layers; ++l) {
    mix(o_tpw[l]);
    mix(o_wk[l]);
    mix(o_wt[l]);
    mixm(latent[l]);
  }
  mixm(embed);
  mixm(readout);
  return h ? h : 1;
}

struct aa_model_plan {
  aa_model_config cfg;               // at the widened sizes of `pipe`
  aa_plan_options opt{};
  ModelPipeline pipe{};              // what the plan runs: set by choose_pipeline in aa_model_plan_create, read everywhere else
  int D, R, W, SL1;  // SH dim, irreps, env weight numel, S*(L+1)
  std::vector<std::vector<int32_t>> keep_i32;
  std::vector<std::vector<double>> keep_f64;
  std::vector<TpLayerDev> layers;
  std::vector<void*> owned;
  BlobLayout blob;                   // where each weight lies in the packed blob: set once by layout_blob in aa_model_plan_create, read everywhere else
  int u_raw;                         // num_tensor_features of the model; cfg.num_tensor is the next multiple of 64 when the channels were padded
  int hid_raw[3];                    // hidden widths of scalar_embed_mlp / latent MLPs / edge_readout in the model (cfg holds the padded ones)
  mutable bool taps = false;         // aa_model_plan_enable_taps: staged pipeline so that every tap is materialised
  size_t esize() const { return cfg.dtype == AA_F32 ? 4 : 8; }
  // optional hipGraph replay of the whole step (aa_model_plan_enable_graph): the launch sequence is captured once per
  // distinct argument set and replayed with one hipGraphLaunch -- for launch-bound (small) systems
  mutable void* ev_wait = nullptr;    // aa_model_plan_set_forward_events
  mutable void* ev_record = nullptr;
  // ZBL pair potential (aa_model_plan_set_pair_zbl): per-type-pair constants [T*T][2] on the device, immutable until set again
  double* zbl_tab = nullptr;
  double zbl_poly_p = 0.0;
  struct StepGraph {
    bool enabled = false;
    hipStream_t cap_stream = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    struct Key {
      const void *weights, *pos, *ws, *e, *f, *center, *nbr, *rowptr, *types, *shift, *trow, *tperm;
      int64_t N, E, a0, a1;
      size_t wsb;
      int64_t max_degree;  // selects the fused forward: part of what was captured
      int64_t taps;        // aa_model_plan_enable_taps switches pipelines
      bool operator==(const Key& o) const { return std::memcmp(this, &o, sizeof(Key)) == 0; }
    } key{};
  };
  mutable StepGraph sg;
  // Host-visible status word (pinned host memory, written by kernels, read by the host without a synchronisation): a step
  // whose graph contradicts the caller's hints (aa_graph.max_degree, atom_begin / atom_end) sets it, the offending atoms'
  // energies become NaN, and the NEXT aa_model_energy_forces on the plan -- or aa_model_check, which synchronises first --
  // returns AA_ERR_INVALID.  > 0: degree of a center atom beyond max_degree; -2: edges outside [atom_begin, atom_end);
  // <= -16: block -16 - v of a blocked step was cut at the wrong edge; <= kFrameStatusBase: frame kFrameStatusBase - v of a per-frame
  // sum (aa_model_frame_*) had offsets the kernel had to clamp.
  int32_t* status = nullptr;
};

// reads and clears the status word; AA_OK when clean
static int consume_status(const aa_model_plan* plan, const char* who) {
  if (!plan->status) return AA_OK;
  // read-and-clear in ONE atomic exchange: a violation a kernel of another stream writes between a separate read and clear would be
  // lost.  (The word is per plan: with several host threads stepping one plan a violation is reported to whichever of them looks
  // first -- include/allegro_amd.h, aa_model_check -- so a host that needs attribution uses one plan per stepping thread.)
  if (*reinterpret_cast<volatile int32_t*>(plan->status) == 0) return AA_OK;
  const int32_t v = __atomic_exchange_n(plan->status, 0, __ATOMIC_ACQ_REL);
  if (v == 0) return AA_OK;
  char msg[384];
  if (v > 0)
    snprintf(msg, sizeof msg, "%s: a step on this plan met a center atom with %d edges, more than aa_graph.max_degree promised "
             "(its energy was set to NaN; pass the true maximum, or 0 for \"unknown\")", who, int(v));
  else if (v <= kFrameStatusBase)
    snprintf(msg, sizeof msg, "%s: a per-frame sum on this plan was given offsets outside [0, num_atoms] or decreasing for frame %d: "
             "aa_frames.frame_atoms[b] / frame_atoms[b + 1] were clamped (that frame's row was set to NaN)", who, int(kFrameStatusBase - v));
  else if (v <= -16)
    snprintf(msg, sizeof msg, "%s: a blocked step on this plan was given a wrong cut for block %d: block_edges[b] / block_edges[b + 1] are not "
             "rowptr[block_atoms[b]] / rowptr[block_atoms[b + 1]] (energies and forces of the frame were set to NaN)", who, int(-16 - v));
  else
    snprintf(msg, sizeof msg, "%s: a step on this plan met edges whose center lies outside [aa_graph.atom_begin, atom_end)", who);
  return fail(AA_ERR_INVALID, msg);
}

static int validate_config(const aa_model_config* cfg) {
  AA_REQUIRE(cfg->dtype == AA_F32 || cfg->dtype == AA_F64, "model: bad dtype");
  AA_REQUIRE(cfg->l_max >= 1 && cfg->l_max <= 3, "model: l_max must be 1..3");
  for (int i = 0; i < 3; ++i) AA_REQUIRE(cfg->act_kind[i] >= AA_ACT_SILU && cfg->act_kind[i] <= AA_ACT_NONE, "model: unknown nonlinearity");
  AA_REQUIRE(cfg->num_layers >= 1 && cfg->num_layers <= AA_MAX_LAYERS, "model: num_layers out of range");
  AA_REQUIRE(cfg->embed_mlp_depth + 1 <= AA_MAX_MLP_LAYERS && cfg->latent_mlp_depth + 1 <= AA_MAX_MLP_LAYERS &&
                 cfg->readout_mlp_depth + 1 <= AA_MAX_MLP_LAYERS,
             "model: MLP too deep");
  AA_REQUIRE(cfg->num_types > 0 && cfg->embed_dim % 2 == 0, "model: bad embedding sizes");
  if (cfg->num_bessels < 1 || cfg->num_bessels > kMaxBessel)
    return fail(AA_ERR_INVALID, "model: num_bessels / num_splines = " + std::to_string(cfg->num_bessels) + ", the edge kernels take 1.." +
                                    std::to_string(kMaxBessel) + " radial basis functions");
  AA_REQUIRE(cfg->embed_kind == 0 || (cfg->embed_kind == 1 && cfg->spline_span >= 0 && cfg->spline_span <= cfg->num_bessels),
             "model: embed_kind must be 0 (Bessel) or 1 (spline, 0 <= span <= num_splines)");
  // the LDS tables of the two edge kernels grow with the basis, the embedding width and the species count: a configuration they
  // cannot be launched for is refused here, not by a launch helper behind a forward that has already written energies
  return check_edge_kernel_limits(cfg->dtype == AA_F64 ? 8 : 4, cfg->num_bessels, cfg->embed_dim, cfg->l_max, cfg->num_types);
}

extern "C" int aa_model_plan_create(const aa_model_config* cfg, aa_model_plan** out) {
  return aa_model_plan_create_with_options(cfg, nullptr, out);
}

// validate -> choose_pipeline -> widen the configuration -> build the tensor-product layers -> layout_blob -> status word
extern "C" int aa_model_plan_create_with_options(const aa_model_config* cfg_in, const aa_plan_options* options, aa_model_plan** out) {
  AA_REQUIRE(cfg_in && out, "aa_model_plan_create: null argument");
  if (int rc = validate_config(cfg_in)) return rc;
  aa_model_plan* p = new aa_model_plan();
  p->opt = options ? *options : aa_plan_options{};
  p->pipe = choose_pipeline(*cfg_in, p->opt);
  const ModelPipeline& pipe = p->pipe;
  p->u_raw = cfg_in->num_tensor;
  p->hid_raw[0] = cfg_in->embed_mlp_width;
  p->hid_raw[1] = cfg_in->latent_mlp_width;
  p->hid_raw[2] = cfg_in->readout_mlp_width;
  p->cfg = *cfg_in;  // ... at the widened sizes
  p->cfg.num_tensor = pipe.num_tensor;
  p->cfg.embed_mlp_width = pipe.embed_width;
  p->cfg.latent_mlp_width = pipe.latent_width;
  p->cfg.readout_mlp_width = pipe.readout_width;
  if (pipe.num_tensor != p->u_raw)
    for (int l = 0; l < p->cfg.num_layers; ++l) p->cfg.tps[l].mul = pipe.num_tensor;
  const aa_model_config* cfg = &p->cfg;
  const int L = cfg->num_layers, S = cfg->num_scalar, u = cfg->num_tensor;
  p->R = cfg->l_max + 1;
  p->D = p->R * p->R;
  p->W = p->R * u;
  p->SL1 = S * (L + 1);
  auto bail = [&](int rc) {
    for (void* q : p->owned) (void)hipFree(q);
    delete p;
    return rc;
  };
  p->layers.resize(L);
  for (int l = 0; l < L; ++l) {
    const aa_tp_desc& d = cfg->tps[l];
    bool ok = d.mul == u && d.d2 == p->D && (l == 0 ? d.d1 == p->D : d.d1 == cfg->tps[l - 1].dout) &&
              (l == L - 1 ? d.dout >= 1 : true);
    if (!ok) return bail(fail(AA_ERR_INVALID, "model: tensor-product layer dims are inconsistent"));
    int rc = build_tp_layer(d, &p->layers[l], &p->owned);
    if (rc) return bail(rc);
    // the plan must not keep pointers into the caller's descriptor arrays
    p->cfg.tps[l].nz_i = p->cfg.tps[l].nz_j = p->cfg.tps[l].nz_k = p->cfg.tps[l].nz_path = nullptr;
    p->cfg.tps[l].nz_val = nullptr;
  }
  p->blob = layout_blob(p->cfg, pipe);
  {
    void* st = nullptr;
    if (hipHostMalloc(&st, 64, hipHostMallocDefault) != hipSuccess || !st) {
      aa_model_plan_destroy(p);
      return fail(AA_ERR_HIP, "aa_model_plan_create: cannot allocate the status word");
    }
    std::memset(st, 0, 64);
    p->status = static_cast<int32_t*>(st);
  }
  *out = p;
  return AA_OK;
}

extern "C" int aa_model_plan_describe(const aa_model_plan* p, char* buf, size_t n) {
  AA_REQUIRE(p && buf && n > 0, "aa_model_plan_describe: null argument");
  const ModelPipeline& m = p->pipe;
  const bool fused = m.fused_fwd;
  // MFMA steps (one step = a 64-feature tile pair x a 32-deep chunk = 24 bf16 MFMAs per 32-edge tile) of the fused forward: executed
  // (after the folds) vs the step-equivalents of the reference's linear layers (what `roofline.achieved` prices)
  const int R = p->R;
  const int ref_steps = 2 + 2 + (2 + 2 * R) + 4 + 2 + 6 + 2 + 6;
  const int exec_steps = fused ? fused_fwd_num_steps(R) - 8 /* env-projection steps: vector work */ : 0;
  const int k = snprintf(buf, n,
                         "{\"fused_forward\": %s, \"fold_embed_table\": %s, \"fold_embed_output\": %s, \"fold_latent_outputs\": %s, "
                         "\"fold_lat0_reverse\": %s, \"fused_mfma_steps_executed\": %d, \"fused_mfma_steps_reference\": %d, "
                         "\"chain_gemm\": %s, \"moments\": %s, \"operator_path\": %s, \"slot_form\": %s, \"fused_wide\": %s%s}",
                         fused ? "true" : "false", (fused && m.fold_embed_table) ? "true" : "false",
                         (fused && m.fold_embed_output) ? "true" : "false", (fused && m.fold_latent_outputs) ? "true" : "false",
                         m.fold_lat0_reverse ? "true" : "false", exec_steps, fused ? ref_steps : 0, m.chains() ? "true" : "false",
                         m.env_moments() ? "true" : "false", m.tp == TpPath::Operator ? "true" : "false", m.slot() ? "true" : "false",
                         m.fused_wide ? "true" : "false", p->zbl_tab ? ", \"pair\": \"zbl\"" : "");
  return (k < 0 || size_t(k) >= n) ? fail(AA_ERR_INVALID, "aa_model_plan_describe: buffer too small") : k;
}

extern "C" int aa_model_check(const aa_model_plan* plan, aa_stream stream) {
  AA_REQUIRE(plan, "aa_model_check: null plan");
  AA_CHECK_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return consume_status(plan, "aa_model_check");
}

extern "C" int aa_model_plan_set_forward_events(aa_model_plan* plan, void* wait_event, void* record_event) {
  AA_REQUIRE(plan, "aa_model_plan_set_forward_events: null plan");
  plan->ev_wait = wait_event;
  plan->ev_record = record_event;
  return AA_OK;
}

static void drop_step_graph(aa_model_plan* plan) {
  aa_model_plan::StepGraph& g = plan->sg;
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr;
  g.graph = nullptr;
}

extern "C" int aa_model_plan_set_pair_zbl(aa_model_plan* plan, const aa_pair_zbl* zbl) {
  AA_REQUIRE(plan, "aa_model_plan_set_pair_zbl: null plan");
  double* tab = nullptr;
  if (zbl) {
    const int T = plan->cfg.num_types;
    AA_REQUIRE(zbl->num_types == T, "aa_model_plan_set_pair_zbl: num_types differs from the plan's");
    AA_REQUIRE(zbl->atomic_numbers, "aa_model_plan_set_pair_zbl: null atomic_numbers");
    for (int t = 0; t < T; ++t) AA_REQUIRE(zbl->atomic_numbers[t] > 0.0, "aa_model_plan_set_pair_zbl: atomic numbers must be positive");
    AA_REQUIRE(zbl->qqr2e > 0.0, "aa_model_plan_set_pair_zbl: qqr2e must be positive");
    AA_REQUIRE(zbl->poly_p > 0.0, "aa_model_plan_set_pair_zbl: poly_p must be positive");
    std::vector<double> host(size_t(T) * T * 2);
    for (int i = 0; i < T; ++i)
      for (int j = 0; j < T; ++j) {
        const double zi = zbl->atomic_numbers[i], zj = zbl->atomic_numbers[j];
        host[2 * (size_t(i) * T + j)] = (std::pow(zi, 0.23) + std::pow(zj, 0.23)) / 0.46850;
        host[2 * (size_t(i) * T + j) + 1] = 0.5 * zbl->qqr2e * zi * zj;
      }
    AA_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&tab), host.size() * sizeof(double)));
    if (hipMemcpy(tab, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(tab);
      return fail(AA_ERR_HIP, "aa_model_plan_set_pair_zbl: cannot copy the pair table");
    }
  }
  // a captured step belongs to the pair potential that was set when it was captured; steps still in flight read the old table
  // (hipFree waits for them)
  drop_step_graph(plan);
  if (plan->zbl_tab) (void)hipFree(plan->zbl_tab);
  plan->zbl_tab = tab;
  plan->zbl_poly_p = zbl ? zbl->poly_p : 0.0;
  return AA_OK;
}

extern "C" int aa_model_plan_enable_graph(aa_model_plan* plan, int on) {
  AA_REQUIRE(plan, "aa_model_plan_enable_graph: null plan");
  aa_model_plan::StepGraph& g = plan->sg;
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr;
  g.graph = nullptr;
  g.enabled = on != 0;
  if (g.enabled && !g.cap_stream) AA_CHECK_HIP(hipStreamCreateWithFlags(&g.cap_stream, hipStreamNonBlocking));
  return AA_OK;
}

extern "C" int aa_model_plan_enable_taps(aa_model_plan* plan, int on) {
  AA_REQUIRE(plan, "aa_model_plan_enable_taps: null plan");
  plan->taps = on != 0;
  // a captured step belongs to the pipeline that was selected when it was captured
  aa_model_plan::StepGraph& g = plan->sg;
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr;
  g.graph = nullptr;
  return AA_OK;
}

extern "C" void aa_model_plan_destroy(aa_model_plan* plan) {
  if (!plan) return;
  if (plan->sg.exec) (void)hipGraphExecDestroy(plan->sg.exec);
  if (plan->sg.graph) (void)hipGraphDestroy(plan->sg.graph);
  if (plan->sg.cap_stream) (void)hipStreamDestroy(plan->sg.cap_stream);
  for (void* q : plan->owned) (void)hipFree(q);
  if (plan->zbl_tab) (void)hipFree(plan->zbl_tab);
  if (plan->status) (void)hipHostFree(plan->status);
  delete plan;
}

extern "C" size_t aa_model_weights_bytes(const aa_model_plan* plan) { return plan ? plan->blob.n_elems * plan->esize() : 0; }

extern "C" uint64_t aa_model_plan_layout_hash(const aa_model_plan* p) { return p ? p->blob.hash(p->cfg, p->pipe, p->u_raw) : 0; }

// alpha_i of nequip ScalarMLPFunction: c_prev / sqrt(fan_in | fan_out)
// `which`: 0 scalar_embed_mlp, 1 latent MLPs, 2 edge_readout (their nonlinearities may differ); linear maps pass -1
static double act_const_of(const aa_model_config& c, int which) {
  if (which < 0) return 1.0;
  if (c.act_kind[which] == AA_ACT_NONE) return 1.0;
  return c.act_consts[which] > 0 ? c.act_consts[which] : c.act_const;
}
static double mlp_alpha(const aa_model_config& c, int layer, int din, int dout, int which = -1) {
  double norm = layer == 0 ? 1.0 : act_const_of(c, which);
  return norm / std::sqrt(double(c.forward_weight_init ? din : dout));
}

// ------------------------------------------------------------------------------------------------
// packing: raw state_dict tensors -> the blob (host arithmetic only: pack_blob_host), then one upload (aa_model_pack_weights)
// ------------------------------------------------------------------------------------------------
// C[M,N] = A[M,K] . B[K,N] in fp64, row-major with leading dimensions lda / ldb.  Every element of C is ONE accumulator that starts at
// 0.0 and takes A[i][k] * B[k][j] in ascending k -- the blob is pinned byte by byte (tests/test_weight_blob.py), so no blocking and
// no pairwise sums here.  (k is the middle loop only so that B is read along its rows.)
static std::vector<double> matmul(const double* A, int lda, const double* B, int ldb, int M, int K, int N) {
  std::vector<double> C(size_t(M) * N, 0.0);
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < K; ++k) {
      const double a = A[size_t(i) * lda + k];
      for (int j = 0; j < N; ++j) C[size_t(i) * N + j] += a * B[size_t(k) * ldb + j];
    }
  return C;
}

// [M,N] row-major -> [N,M]
static std::vector<double> transposed(const double* A, int M, int N) {
  std::vector<double> t(size_t(M) * N);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) t[size_t(j) * M + i] = A[size_t(i) * N + j];
  return t;
}

// One pack: the plan's layout (read only), the caller's tensors, and the blob in fp64 while it is being filled.  run() is the
// sequence of steps; each step writes entries of the layout and reads only raw tensors or entries an earlier step wrote.
struct Packer {
  const aa_model_plan& p;
  aa_model_raw_weights raw;  // the caller's tensors; zero-padded copies (pad_store) where the plan is wider than the model
  const BlobLayout& b = p.blob;
  const aa_model_config& c = p.cfg;
  const ModelPipeline& pipe = p.pipe;
  const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, T = c.num_types, B = c.num_bessels, S0 = c.embed_dim, R = p.R, W = p.W;
  // env-weight columns: reference layout [u][R] (_channels.py:46-51); the specialised kernels want [R][u].
  // With weight_individual_irreps=False the Allegro layers' env weights are [u] in the reference (_channels.py:29-31,
  // 60-63: one weight per channel for all irreps): the packed matrices replicate that column for every irrep, which
  // is the same linear map, so every kernel runs unchanged.  (The tensor-embedding weights w0 are always individual,
  // tensorembed.py:76-81.)
  const bool shared = c.env_shared_weights != 0;
  const int We_in = shared ? p.u_raw : R * p.u_raw, We = shared ? u : W;  // env-weight columns of first_proj / latent outputs in the state_dict, and zero-padded to the plan's channels
  // how much wider the plan's (padded) shapes are than the model's: the ScalarMLPFunction constants (alpha = c / sqrt(fan_in | fan_out))
  // keep following the TRUE layer shapes
  const int du = u - p.u_raw, dW = W - R * p.u_raw, dWe = We - We_in, dHe = c.embed_mlp_width - p.hid_raw[0],
            dHl = c.latent_mlp_width - p.hid_raw[1], dHr = c.readout_mlp_width - p.hid_raw[2];
  std::vector<std::vector<double>> pad_store;
  std::vector<double> stage;  // fp32 plans: the fp64 blob before rounding (fp64 plans fill the output bytes directly)
  double* h = nullptr;        // the blob in fp64, b.n_elems elements, zero where nothing is written
  std::vector<double> g0f, wenv0f;         // fold_embed_output(): W1 @ G0 [He, ng0] and W1 @ Wenv0 [He, R u]
  std::vector<const GemmMat*> slot_mats;   // (fp32 plans: their bf16x3 copies are split off the rounded matrices)
  std::vector<const GemmMatSet*> proj_sets;

  void put(size_t off, const double* src, size_t n, double scale) {
    for (size_t i = 0; i < n; ++i) h[off + i] = src[i] * scale;
  }
  // a [rows, cols] product and its transpose
  void put_with_transpose(size_t off, size_t off_t, const std::vector<double>& m, int rows, int cols) {
    std::copy(m.begin(), m.end(), h + off);
    const std::vector<double> t = transposed(m.data(), rows, cols);
    std::copy(t.begin(), t.end(), h + off_t);
  }
  int w0_col(int q) const { return pipe.channel_minor() ? (q % u) * R + q / u : q; }  // packed col q <- reference col
  int env_col(int q) const {
    const int ch = pipe.channel_minor() ? q % u : q / R, r = pipe.channel_minor() ? q / u : q % R;
    return shared ? ch : ch * R + r;
  }

  // zero-extend a row-major [r_raw][c_raw] matrix to [r_pad][c_pad] (every padded block is a suffix: both env layouts are
  // channel-major -- [u][R] or [u] -- and hidden units / scalar rows are appended at the end)
  const double* pad2d(const double* src, int r_raw, int c_raw, int r_pad, int c_pad) {
    if (r_raw == r_pad && c_raw == c_pad) return src;
    pad_store.emplace_back(size_t(r_pad) * c_pad, 0.0);
    std::vector<double>& d = pad_store.back();
    for (int r = 0; r < r_raw; ++r)
      for (int q = 0; q < c_raw; ++q) d[size_t(r) * c_pad + q] = src[size_t(r) * c_raw + q];
    return d.data();
  }

  // Channel-padded plan (choose_pipeline): the state_dict tensors carry u_raw channels; build zero-padded copies in
  // the reference's own layouts so that everything below indexes a u-channel model.
  int pad_raw() {
    if (!(du || dHe || dHl || dHr)) return AA_OK;
    const aa_model_raw_weights in = raw;
    const int u_raw = p.u_raw, dlat = c.latent_mlp_depth, H = c.latent_mlp_width;
    AA_REQUIRE(in.env_embed_linear && in.first_proj, "pack: missing embedding weights");
    raw.env_embed_linear = pad2d(in.env_embed_linear, S, R * u_raw, S, W);
    raw.first_proj = pad2d(in.first_proj, S, S + We_in, S, S + We);
    if (dHe) {  // (only single-hidden-layer MLPs are padded)
      AA_REQUIRE(in.embed_mlp[0] && in.embed_mlp[1], "pack: missing scalar_embed_mlp weights");
      raw.embed_mlp[0] = pad2d(in.embed_mlp[0], S0, p.hid_raw[0], S0, c.embed_mlp_width);
      raw.embed_mlp[1] = pad2d(in.embed_mlp[1], p.hid_raw[0], S, c.embed_mlp_width, S);
    }
    for (int l = 0; l < L; ++l) {
      AA_REQUIRE(in.latent[l][0] && in.latent[l][dlat] && in.tp_weights[l], "pack: missing latent / tp weights");
      const int out_raw = S + (l < L - 1 ? We_in : 0), out_pad = S + (l < L - 1 ? We : 0);
      if (dlat == 0) {
        raw.latent[l][0] = pad2d(in.latent[l][0], S * (l + 1) + u_raw, out_raw, S * (l + 1) + u, out_pad);
      } else {
        // first layer: input rows [S (l + 1) | u scalars], output = hidden units; last layer: [hidden][S | env columns]
        const int H_raw = dlat == 1 ? p.hid_raw[1] : H;
        raw.latent[l][0] = pad2d(in.latent[l][0], S * (l + 1) + u_raw, H_raw, S * (l + 1) + u, H);
        raw.latent[l][dlat] = pad2d(in.latent[l][dlat], H_raw, out_raw, H, out_pad);
      }
      if (c.tps[l].coupling) raw.tp_weights[l] = pad2d(in.tp_weights[l], u_raw, c.tps[l].num_paths, u, c.tps[l].num_paths);
    }
    if (dHr) {
      AA_REQUIRE(in.readout[0] && in.readout[1], "pack: missing readout weights");
      raw.readout[0] = pad2d(in.readout[0], p.SL1, p.hid_raw[2], p.SL1, c.readout_mlp_width);
      raw.readout[1] = pad2d(in.readout[1], p.hid_raw[2], 1, c.readout_mlp_width, 1);
    }
    return AA_OK;
  }

  // cutoffs, radial basis, type embedding; the two-body table where the pipeline carries one
  int pack_embedding() {
    AA_REQUIRE(raw.rmax_recip && raw.env_embed_linear && raw.first_proj, "pack: missing embedding weights");
    put(b.o_rmax, raw.rmax_recip, size_t(T) * T, 1.0);
    if (c.embed_kind == 1) {
      // [class][c][s] (spline.py:69-71) -> basis-major [class][s][c]
      AA_REQUIRE(raw.spline_weights, "pack: missing spline weights");
      for (int cls = 0; cls < T * T; ++cls)
        for (int cc = 0; cc < S0; ++cc)
          for (int n = 0; n < B; ++n) h[b.o_embtab + (size_t(cls) * B + n) * S0 + cc] = raw.spline_weights[(size_t(cls) * S0 + cc) * B + n];
      return AA_OK;
    }
    AA_REQUIRE(raw.bessel_weights && raw.center_embed && raw.neighbor_embed && raw.basis_linear, "pack: missing embedding weights");
    // Two published conventions of nequip's BesselEdgeLengthEncoding (EXT; which one a given nequip release uses
    // cannot be checked in this container -- DESIGN.md section 6): (a) bessel_weights = n pi, basis sin(w x) / x;
    // (b) bessel_weights = n (linspace(1, B, B)), basis sinc(x w) w = sin(pi w x) / (pi x).  Both are served by the
    // same kernels, sin(w' x) / x: (b) is recognised by its integer roots and packed as w' = pi w with the 1/pi
    // prefactor folded into the basis_linear rows.
    const double kPi = 3.14159265358979323846;
    bool sinc_form = c.bessel_convention == 2;
    if (c.bessel_convention == 0) {
      bool is_n = true, is_npi = true;
      for (int n = 0; n < B; ++n) {
        // (relative 1e-5: the roots of an fp32 state_dict are n*pi rounded to fp32)
        is_n = is_n && std::fabs(raw.bessel_weights[n] - double(n + 1)) < 1e-5 * double(n + 1);
        is_npi = is_npi && std::fabs(raw.bessel_weights[n] - double(n + 1) * kPi) < 1e-5 * double(n + 1) * kPi;
      }
      if (!is_n && !is_npi)
        return fail(AA_ERR_INVALID, "pack: bessel_weights are neither n nor n*pi (trained roots?): state aa_model_config.bessel_convention (1: sin(w x)/x, 2: sinc)");
      sinc_form = is_n;
    } else if (c.bessel_convention != 1 && c.bessel_convention != 2) {
      return fail(AA_ERR_INVALID, "pack: bessel_convention must be 0 (recognise), 1 (roots n*pi) or 2 (sinc form)");
    }
    put(b.o_bessel, raw.bessel_weights, B, sinc_form ? kPi : 1.0);
    put(b.o_cemb, raw.center_embed, size_t(T) * S0 / 2, 1.0);
    put(b.o_nemb, raw.neighbor_embed, size_t(T) * S0 / 2, 1.0);
    put(b.o_basis, raw.basis_linear, size_t(B) * S0, mlp_alpha(c, 0, B, S0) * (sinc_form ? 1.0 / kPi : 1.0));
    if (pipe.two_body_table) {
      const int half = S0 / 2;
      for (int ti = 0; ti < T; ++ti)
        for (int tj = 0; tj < T; ++tj)
          for (int n = 0; n < B; ++n)
            for (int cc = 0; cc < S0; ++cc) {
              const double te = cc < half ? h[b.o_cemb + size_t(ti) * half + cc] : h[b.o_nemb + size_t(tj) * half + (cc - half)];
              h[b.o_embtab + ((size_t(ti) * T + tj) * B + n) * S0 + cc] = te * h[b.o_basis + size_t(n) * S0 + cc];
            }
    }
    return AA_OK;
  }

  // pack an MLP; if env_off >= 0 the LAST layer's columns [env_off, env_off+W) are env weights
  // raw_last_width: true column count of the LAST layer in the state_dict (>= packed width when the env columns
  // are split off for the moments path); alpha always follows the reference's full layer shape
  // true_din_less / true_dout_less: how much narrower the reference's first-layer input / last-layer output is than the
  // (channel-padded) shapes packed here -- alpha follows the reference
  // hidden_less: by how much the (single) hidden layer was widened -- layer 0's fan_out and layer 1's fan_in are narrower
  // in the reference.  `total_layers`: layers of the whole MLP (the readout packs only its first ones here).
  bool pack_mlp(const MlpLayout& m, const double* const* ws, int nlayers, int env_off, int which, int raw_last_width = -1,
                int true_din_less = 0, int true_dout_less = 0, int hidden_less = 0, int total_layers = -1) {
    if (total_layers < 0) total_layers = nlayers;
    for (int i = 0; i < nlayers; ++i) {
      if (!ws[i]) return false;
      int din = m.dims[i], dout = m.dims[i + 1];
      int raw_w = (i == nlayers - 1 && raw_last_width > 0) ? raw_last_width : dout;
      double al = mlp_alpha(c, i, din - (i == 0 ? true_din_less : hidden_less),
                            raw_w - (i == total_layers - 1 ? true_dout_less : hidden_less), which);
      for (int r = 0; r < din; ++r)
        for (int q = 0; q < dout; ++q) {
          int src = q;
          if (i == nlayers - 1 && env_off >= 0 && q >= env_off && q < env_off + W) src = env_off + env_col(q - env_off);
          double v = ws[i][size_t(r) * raw_w + src] * al;
          h[m.w[i] + size_t(r) * dout + q] = v;
          h[m.wt[i] + size_t(q) * din + r] = v;
        }
      gemm_pack_b(&h[m.w[i]], din, dout, &h[m.wp[i]]);
      gemm_pack_b(&h[m.wt[i]], dout, din, &h[m.wtp[i]]);
    }
    return true;
  }

  // fused first stage: [ two_body (first_proj[:, :S]) | w0 (env_embed_linear) | env_w0 (first_proj[:, S:]) ]
  // (moments path: the env_w0 columns are not part of the GEMM; they become Wenv of layer 0, pack_env_weights)
  void pack_first_stage() {
    const int NG = b.ng0;
    double a_env = mlp_alpha(c, 0, S, W - dW), a_proj = mlp_alpha(c, 0, S, S + We - dWe);
    for (int r = 0; r < S; ++r)
      for (int q = 0; q < NG; ++q) {
        double v;
        if (q < S)
          v = raw.first_proj[size_t(r) * (S + We) + q] * a_proj;
        else if (q < S + W)
          v = raw.env_embed_linear[size_t(r) * W + w0_col(q - S)] * a_env;
        else
          v = raw.first_proj[size_t(r) * (S + We) + S + env_col(q - S - W)] * a_proj;
        h[b.o_g0 + size_t(r) * NG + q] = v;
        h[b.o_g0t + size_t(q) * S + r] = v;
      }
    gemm_pack_b(&h[b.o_g0], S, NG, &h[b.o_g0p]);
    gemm_pack_b(&h[b.o_g0t], NG, S, &h[b.o_g0tp]);
  }

  // the three MLP stacks with the ScalarMLPFunction constants applied, the first stage, tensor-product weights, scales and shifts
  int pack_mlps() {
    AA_REQUIRE(pack_mlp(b.embed, raw.embed_mlp, c.embed_mlp_depth + 1, -1, 0, -1, 0, 0, dHe), "pack: missing scalar_embed_mlp weights");
    pack_first_stage();
    for (int l = 0; l < L; ++l) {
      AA_REQUIRE(pack_mlp(b.latent[l], raw.latent[l], c.latent_mlp_depth + 1, (l < L - 1 && !pipe.env_moments()) ? S : -1, 1,
                          S + (l < L - 1 ? We : 0), du, l < L - 1 ? dWe : 0, dHl),
                 "pack: missing latent weights");
      AA_REQUIRE(raw.tp_weights[l], "pack: missing tp weights");
      put(b.o_tpw[l], raw.tp_weights[l], size_t(c.tps[l].coupling ? u : 1) * c.tps[l].num_paths, 1.0);
    }
    pack_env_weights();
    AA_REQUIRE(pack_mlp(b.readout, raw.readout, c.readout_mlp_depth, -1, 2, -1, 0, 0, dHr, c.readout_mlp_depth + 1), "pack: missing readout weights");
    const double* wl = raw.readout[c.readout_mlp_depth];
    AA_REQUIRE(wl, "pack: missing readout weights");
    put(b.o_ro_last, wl, b.ro_last_dim, mlp_alpha(c, c.readout_mlp_depth, b.ro_last_dim - (c.readout_mlp_depth > 0 ? dHr : 0), 1, 2));
    if (c.has_scales) {
      AA_REQUIRE(raw.scales, "pack: missing scales");
      put(b.o_scales, raw.scales, T, 1.0);
    }
    if (c.has_shifts) {
      AA_REQUIRE(raw.shifts, "pack: missing shifts");
      put(b.o_shifts, raw.shifts, T, 1.0);
    }
    return AA_OK;
  }

  // (moments / operator plans) Wenv_l[k][r][ch] and its [r][ch][k] transpose from the reference's [k][S + ch*R + r] columns
  void pack_env_weights() {
    if (!pipe.env_moments()) return;
    auto fill = [&](int l, const double* rawm, int ka, int raw_w, double al) {
      for (int k = 0; k < ka; ++k)
        for (int r = 0; r < R; ++r)
          for (int ch = 0; ch < u; ++ch) {
            double v = rawm[size_t(k) * raw_w + S + (shared ? ch : ch * R + r)] * al;
            h[b.o_wk[l] + (size_t(k) * R + r) * u + ch] = v;
            h[b.o_wt[l] + (size_t(r) * u + ch) * ka + k] = v;
          }
    };
    fill(0, raw.first_proj, S, S + We, mlp_alpha(c, 0, S, S + We - dWe));
    const int dl = c.latent_mlp_depth;  // index of a latent's last layer
    for (int l = 1; l < L; ++l)
      fill(l, raw.latent[l - 1][dl], c.latent_mlp_width, S + We, mlp_alpha(c, dl, c.latent_mlp_width - dHl, S + We - dWe, 1));
  }

  // The output layer W1 [He, S] of scalar_embed_mlp folded into its two consumers, formed once for the chains pipeline
  // (fold_embed_output, He = 64) and the slot form (He = S): W1 @ G0 and Wenv0'[k][r][ch] = sum_m W1[k][m] Wenv0[m][r][ch]
  void fold_embed_output() {
    const int De = c.embed_mlp_depth;
    const double* w1 = &h[b.embed.w[De]];
    g0f = matmul(w1, S, &h[b.o_g0], b.ng0, b.embed.dims[De], S, b.ng0);
    wenv0f = matmul(w1, S, &h[b.o_wk[0]], W, b.embed.dims[De], S, W);
  }

  // F(j -> consumer) = Wout_j [H, S] @ Wc[S (j+1) .. S (j+2)) [S, Nc]: the consumer's row block of lat_j behind latent j's output layer
  std::vector<double> fold_block(int j, const double* wc, int Nc) const {
    return matmul(&h[b.latent[j].w[1]], S, wc + size_t(S) * (j + 1) * Nc, Nc, c.latent_mlp_width, S, Nc);
  }
  // ... in place, in a copy f [., Nc] of the consumer's first layer (S = H wherever a layer is folded, so the block keeps its size)
  void fold_rows(std::vector<double>& f, int j, int Nc) const {
    const std::vector<double> blk = fold_block(j, f.data(), Nc);
    std::copy(blk.begin(), blk.end(), f.begin() + size_t(S) * (j + 1) * Nc);
  }

  // (fp64 part of the chains pipeline's folds; the bf16x3 ones follow the rounding: pack_chain_folds)
  void pack_embed_folds() {
    if (pipe.fold_embed_output) put_with_transpose(b.o_wk0f, b.o_wt0f, wenv0f, 64, W);  // as [k][R][u] and [R][u][k]
    if (pipe.fold_embed_table) {
      // T[pair][n][k] = sum_c tab[pair][n][c] * W0[c][k]  (W0: the packed first layer of scalar_embed_mlp, normalisation folded)
      const int H = b.embed.dims[1];
      const std::vector<double> t = matmul(&h[b.o_embtab], S0, &h[b.embed.w[0]], H, T * T * B, S0, H);
      std::copy(t.begin(), t.end(), h + b.o_embtab_h);
    }
  }

  void put_slot(const GemmMat& m, const std::vector<double>& d) {
    std::copy(d.begin(), d.end(), h + m.w);
    gemm_pack_b(&h[m.w], m.K, m.N, &h[m.wp]);
    slot_mats.push_back(&m);
  }

  // slot form: every matrix below is a product / regrouping of the NORMALISED matrices packed above, formed in fp64
  void pack_slot_form() {
    const int Hr = c.readout_mlp_width, H = c.latent_mlp_width, NG = b.ng0, SL1 = p.SL1;
    put_slot(b.s_g0f, g0f);
    put_slot(b.s_g0ft, transposed(g0f.data(), S, NG));
    put_with_transpose(b.o_s_wk0, b.o_s_wt0, wenv0f, S, W);
    // forward: first layers with the row blocks of the earlier latents folded; the tensor scalars' rows, transposed
    for (int l = 0; l < L; ++l) {
      const int K = S * (l + 1) + u;
      const double* win = &h[b.latent[l].w[0]];  // [K, H]
      std::vector<double> f(win, win + size_t(K) * H);
      for (int j = 0; j < l; ++j) fold_rows(f, j, H);
      put_slot(b.s_in[l], f);
      put_slot(b.s_sct[l], transposed(win + size_t(S) * (l + 1) * H, u, H));
    }
    const double* wro = &h[b.readout.w[0]];  // [SL1, Hr]
    std::vector<double> ro0(wro, wro + size_t(SL1) * Hr);
    for (int j = 0; j < L; ++j) fold_rows(ro0, j, Hr);
    put_slot(b.s_ro0, ro0);
    // reverse, by slot: rows follow the operand [d readout hidden | d z_{l+1} .. d z_{L-1}], columns the hidden units of latent l
    for (int l = 0; l < L; ++l) {
      std::vector<double> rs = transposed(fold_block(l, wro, Hr).data(), H, Hr);
      for (int l2 = l + 1; l2 < L; ++l2) {
        const std::vector<double> t = transposed(fold_block(l, &h[b.latent[l2].w[0]], H).data(), H, H);
        rs.insert(rs.end(), t.begin(), t.end());
      }
      put_slot(b.s_rs[l], rs);
    }
    // ... and slot 0 (two-body): the two-body rows of the readout's and of every latent's first layer, transposed
    std::vector<double> tb = transposed(wro, S, Hr);
    for (int l2 = 0; l2 < L; ++l2) {
      const std::vector<double> t = transposed(&h[b.latent[l2].w[0]], S, H);
      tb.insert(tb.end(), t.begin(), t.end());
    }
    put_slot(b.s_rstb, tb);
  }

  // operator-kernel plans: per layer the R matrices f Wenv_l[:, r, :] [ka, u] and their transposes, f = 1 / sqrt(avg_num_neighbors)
  void pack_proj_sets() {
    const double sf = 1.0 / std::sqrt(c.avg_num_neighbors);
    auto put_set = [&](const GemmMatSet& fw, const GemmMatSet& bw, size_t wk_off, int ka) {
      for (int r = 0; r < R; ++r) {
        for (int k = 0; k < ka; ++k)
          for (int ch = 0; ch < u; ++ch) {
            const double v = sf * h[wk_off + (size_t(k) * R + r) * u + ch];
            h[fw.w + r * fw.w_bs + size_t(k) * u + ch] = v;
            h[bw.w + r * bw.w_bs + size_t(ch) * ka + k] = v;
          }
        gemm_pack_b(&h[fw.w + r * fw.w_bs], ka, u, &h[fw.wp + r * fw.wp_bs]);
        gemm_pack_b(&h[bw.w + r * bw.w_bs], u, ka, &h[bw.wp + r * bw.wp_bs]);
      }
      proj_sets.push_back(&fw);
      proj_sets.push_back(&bw);
    };
    for (int l = 0; l < L; ++l) put_set(b.s_pr[l], b.s_prt[l], b.o_wk[l], l == 0 ? S : c.latent_mlp_width);
    if (pipe.slot()) put_set(b.s_pr0f, b.s_prt0f, b.o_s_wk0, S);
  }

  // fp32 plans: round the blob once, then split the bf16x3 copies off the ROUNDED matrices (bit patterns stored in float slots)
  void round_and_split(float* hf) {
    for (size_t i = 0; i < b.n_elems; ++i) hf[i] = float(h[i]);
    auto splitw = [&](size_t w_off, int K, int N, size_t q_off) {
      gemm_pack_bf16x3(&hf[w_off], K, N, reinterpret_cast<unsigned*>(&hf[q_off]));
    };
    auto split_mlp = [&](const MlpLayout& m, int nlayers) {
      for (int i = 0; i < nlayers; ++i) {
        splitw(m.w[i], m.dims[i], m.dims[i + 1], m.wq[i]);
        splitw(m.wt[i], m.dims[i + 1], m.dims[i], m.wtq[i]);
      }
    };
    split_mlp(b.embed, c.embed_mlp_depth + 1);
    splitw(b.o_g0, S, b.ng0, b.o_g0q);
    splitw(b.o_g0t, b.ng0, S, b.o_g0tq);
    for (int l = 0; l < L; ++l) split_mlp(b.latent[l], c.latent_mlp_depth + 1);
    split_mlp(b.readout, c.readout_mlp_depth);
    for (const GemmMat* m : slot_mats) splitw(m->w, m->K, m->N, m->wq);
    for (const GemmMatSet* m : proj_sets)
      for (int r = 0; r < m->count; ++r) splitw(m->w + r * m->w_bs, m->K, m->N, m->wq + r * m->wq_bs);
  }

  // bf16x3 words of a [K, N] fp64 matrix, rounded to fp32 once
  static void put_bf16x3(const std::vector<double>& m, int K, int N, float* hf, size_t q_off) {
    const std::vector<float> f(m.begin(), m.end());
    gemm_pack_bf16x3(f.data(), K, N, reinterpret_cast<unsigned*>(&hf[q_off]));
  }

  // Chains pipeline (fp32; S = u = every MLP width = 64): the merged reverse chain "readout' o latent_{L-1}'" (Runner::backward) and,
  // 2-layer stacks, the bf16x3 copies of the folded layers.  The folds are formed in fp64 from the normalised matrices and rounded once.
  void pack_chain_folds(float* hf) {
    const int SL = S * L, SL1 = p.SL1, N2 = SL + u;
    const float* rt = &hf[b.readout.wt[0]];        // [64, SL1]  (transposed first readout layer)
    const float* lt = &hf[b.latent[L - 1].wt[0]];  // [64, N2]   (transposed first layer of the last latent)
    // a: readout-reverse columns feeding the last latent; st: [readout-reverse ; latent-reverse] stacked, the columns of the
    // earlier features (d_fcat[:, :SL]); cm: latent-reverse columns of the tensor scalars (d_scal)
    std::vector<float> a(size_t(64) * S), st(size_t(128) * SL), cm(size_t(64) * u);
    for (int k = 0; k < 64; ++k) {
      for (int n = 0; n < S; ++n) a[size_t(k) * S + n] = rt[size_t(k) * SL1 + SL + n];
      for (int n = 0; n < SL; ++n) {
        st[size_t(k) * SL + n] = rt[size_t(k) * SL1 + n];
        st[size_t(64 + k) * SL + n] = lt[size_t(k) * N2 + n];
      }
      for (int n = 0; n < u; ++n) cm[size_t(k) * u + n] = lt[size_t(k) * N2 + SL + n];
    }
    gemm_pack_bf16x3(a.data(), 64, S, reinterpret_cast<unsigned*>(&hf[b.o_b3a_q]));
    gemm_pack_bf16x3(st.data(), 128, SL, reinterpret_cast<unsigned*>(&hf[b.o_b3b_q]));
    gemm_pack_bf16x3(cm.data(), 64, u, reinterpret_cast<unsigned*>(&hf[b.o_b3c_q]));
    if (pipe.fold_embed_output) {  // first stage behind the output layer of scalar_embed_mlp: W1 @ G0 and its transpose
      put_bf16x3(g0f, 64, b.ng0, hf, b.o_g0fq);
      put_bf16x3(transposed(g0f.data(), 64, b.ng0), b.ng0, 64, hf, b.o_g0tfq);
    }
    if (!pipe.fold_latent_outputs) return;
    // folded first layers: row block "lat_l" of a consumer's first layer <- Wout_l @ that block.  Row order of the consumers:
    // [two-body | lat0 | scal1] (latent 1), [two-body | lat0 | lat1] (readout)
    const double* win1 = &h[b.latent[1].w[0]];
    const double* wro = &h[b.readout.w[0]];
    std::vector<double> l1(win1, win1 + size_t(2 * S + u) * 64), r0(wro, wro + size_t(3 * S) * 64);
    fold_rows(l1, 0, 64);
    fold_rows(r0, 0, 64);
    fold_rows(r0, 1, 64);
    put_bf16x3(l1, 2 * S + u, 64, hf, b.o_lat1in_fq);
    put_bf16x3(r0, 3 * S, 64, hf, b.o_ro0_fq);
    // readout-reverse chain: d a1 = d ro_h @ (Wout_1 @ Wro[lat1 rows])^T, one layer instead of two
    put_bf16x3(transposed(&r0[size_t(2 * S) * 64], 64, 64), 64, 64, hf, b.o_b3af_q);
    if (!pipe.fold_lat0_reverse) return;
    // second layer of that chain, [readout' ; latent-1'] -> (d two-body | d lat0): with Wout_0^T folded into the lat0 columns it
    // yields d a_0 (before the moments' share and silu'), and the latent-0 reverse chain needs no output-layer reverse
    std::vector<double> stf(st.begin(), st.end());
    const std::vector<double> lat0 = matmul(&stf[S], SL, &h[b.latent[0].wt[1]], 64, 128, 64, 64);  // [128, lat0 cols] @ Wout_0^T
    for (int k = 0; k < 128; ++k) std::copy(&lat0[size_t(k) * 64], &lat0[size_t(k) * 64] + 64, &stf[size_t(k) * SL + S]);
    put_bf16x3(stf, 128, SL, hf, b.o_b3bf_q);
  }

  // the blob as it will sit in device memory
  int run(std::vector<unsigned char>& bytes) {
    const bool f32 = c.dtype == AA_F32;
    bytes.assign(b.n_elems * p.esize(), 0);
    if (f32) stage.assign(b.n_elems, 0.0);
    h = f32 ? stage.data() : reinterpret_cast<double*>(bytes.data());
    if (int rc = pad_raw()) return rc;
    if (int rc = pack_embedding()) return rc;
    if (int rc = pack_mlps()) return rc;
    if (pipe.fold_embed_output || pipe.slot()) fold_embed_output();
    pack_embed_folds();
    if (pipe.slot()) pack_slot_form();
    if (pipe.op_proj) pack_proj_sets();
    if (f32) {
      float* hf = reinterpret_cast<float*>(bytes.data());
      round_and_split(hf);
      if (pipe.chains()) pack_chain_folds(hf);
    }
    return AA_OK;
  }
};

static int pack_blob_host(const aa_model_plan& p, const aa_model_raw_weights& raw, std::vector<unsigned char>& bytes) {
  return Packer{p, raw}.run(bytes);
}

extern "C" int aa_model_pack_weights(const aa_model_plan* p, const aa_model_raw_weights* raw, void* dev_blob, size_t blob_bytes,
                                     aa_stream stream) {
  AA_REQUIRE(p && raw && dev_blob, "aa_model_pack_weights: null argument");
  AA_REQUIRE(blob_bytes >= aa_model_weights_bytes(p), "aa_model_pack_weights: blob too small");
  std::vector<unsigned char> bytes;
  if (int rc = pack_blob_host(*p, *raw, bytes)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  AA_CHECK_HIP(hipMemcpyAsync(dev_blob, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
  AA_CHECK_HIP(hipStreamSynchronize(s));  // the host staging bytes die at return
  return AA_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace layout
// ------------------------------------------------------------------------------------------------
struct Workspace {
  size_t vec, sh, emb0, emb, w0, fcat, g_fcat, g_envw, g_w0, g_emb, g_emb0, g_sh, g_ro_last, g_aenv, e_edge, q_op, bvec_op, gm_op, mom_op, dx2s_op, trev, dvec, vir_part, tiles;
  size_t g_scal[AA_MAX_LAYERS];
  size_t se_h[AA_MAX_MLP_LAYERS], g_se_h[AA_MAX_MLP_LAYERS];
  size_t envw[AA_MAX_LAYERS], x2s[AA_MAX_LAYERS], tf[AA_MAX_LAYERS], scal[AA_MAX_LAYERS];
  size_t lat_h[AA_MAX_LAYERS][AA_MAX_MLP_LAYERS], g_lat_h[AA_MAX_MLP_LAYERS];
  size_t ro_h[AA_MAX_MLP_LAYERS], g_ro_h[AA_MAX_MLP_LAYERS];
  size_t g_tf[2];
  size_t total;
};

// [E,D] slots that edge_backward sums into d sh: general kernels 1 (accumulated); specialised L+1; operator kernels one
// per 64-channel slice for the x1 path plus one per 64-wide block of every layer's env input
static int num_gsh_slots(const aa_model_plan* p) {
  const aa_model_config& c = p->cfg;
  if (p->pipe.tp_op >= 0) {
    int n = c.num_tensor / 64;
    for (int l = 0; l < c.num_layers; ++l) n += (l == 0 ? c.num_scalar : c.latent_mlp_width) / 64;
    return n;
  }
  return p->pipe.channel_minor() ? c.num_layers + 1 : 1;
}

static Workspace layout_workspace(const aa_model_plan* p, int64_t N, int64_t E, int with_forces) {
  Workspace w{};
  const aa_model_config& c = p->cfg;
  const size_t es = p->esize();
  size_t o = 0;
  auto take = [&](size_t elems) {
    size_t r = o;
    o += (elems * es + 255) / 256 * 256;
    return r;
  };
  const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, S0 = c.embed_dim;
  const size_t Ez = size_t(E), Nz = size_t(N);
  w.vec = take(Ez * 4);
  w.sh = take(Ez * p->D);
  w.emb0 = take(Ez * S0);
  for (int i = 0; i < c.embed_mlp_depth; ++i) w.se_h[i] = take(Ez * c.embed_mlp_width);
  w.emb = take(Ez * S);
  w.w0 = take(Ez * p->W);
  w.fcat = take(Ez * p->SL1);
  size_t dmax = 1;
  for (int l = 0; l < L; ++l) {
    if (!p->pipe.env_moments()) w.envw[l] = take(Ez * p->W);
    w.x2s[l] = take(Nz * u * p->D);
    if (l < L - 1 && p->pipe.chain_pair < 0 && !p->pipe.env_moments()) {
      w.tf[l] = take(Ez * u * c.tps[l].dout);
      dmax = std::max(dmax, size_t(c.tps[l].dout));
    }
    w.scal[l] = take(Ez * u);
    for (int i = 0; i < c.latent_mlp_depth; ++i) w.lat_h[l][i] = take(Ez * c.latent_mlp_width);
  }
  for (int i = 0; i < c.readout_mlp_depth; ++i) w.ro_h[i] = take(Ez * c.readout_mlp_width);
  if (p->pipe.chains()) w.e_edge = take(Ez);
  if (p->pipe.embed_fused) w.trev = take(Ez * 8);
  if (p->pipe.fused_fwd) w.tiles = take(((3 * Nz + 8) * sizeof(int32_t) + es - 1) / es);  // class lists + counters of the team form
  if (with_forces) {
    w.dvec = take(Ez * 4);
    w.vir_part = take((size_t(kVirialBlocks) * 9 * sizeof(double) + es - 1) / es);
  }
  if (p->pipe.tp_op >= 0) {
    w.bvec_op = take(Nz * L * p->D * u);
    w.mom_op = take(Nz * p->D * size_t(std::max(c.num_scalar, c.latent_mlp_width)));
  }
  if (with_forces) {
    w.g_fcat = take(Ez * p->SL1);
    for (int i = 0; i < c.readout_mlp_depth; ++i) w.g_ro_h[i] = take(Ez * c.readout_mlp_width);
    for (int i = 0; i < c.latent_mlp_depth; ++i) w.g_lat_h[i] = take(Ez * c.latent_mlp_width);
    for (int l = 0; l < L; ++l) w.g_scal[l] = take(Ez * u);
    if (!p->pipe.env_moments()) w.g_envw = take(Ez * p->W);
    // (StepPlan::mom0_in_chain: the per-atom GM0 [N][D][64] of the layer-0 moments reverse lies here -- that form never writes d a_e -- so
    //  the slot holds whichever is larger; the same for every step on the plan, whatever form it takes)
    const bool gm0_here = p->pipe.tp == TpPath::Moments && p->pipe.chains() && p->pipe.embed_fused && p->pipe.fold_embed_table && es == 4;
    if (p->pipe.env_moments())
      w.g_aenv = take(std::max(Ez * size_t(std::max(S, c.latent_mlp_width)), gm0_here ? Nz * p->D * 64 : size_t(0)));
    w.g_w0 = take(Ez * p->W);
    if (L > 1 && p->pipe.chain_pair < 0) {
      w.g_tf[0] = take(Ez * u * dmax);
      w.g_tf[1] = L > 2 ? take(Ez * u * dmax) : w.g_tf[0];
    }
    w.g_emb = take(Ez * S);
    for (int i = 0; i < c.embed_mlp_depth; ++i) w.g_se_h[i] = take(Ez * c.embed_mlp_width);
    w.g_emb0 = take(Ez * S0);
    w.g_sh = take(Ez * p->D * num_gsh_slots(p));  // slot 0: x1 path of layer 0; slot l+1: env path of layer l (see num_gsh_slots)
    if (p->pipe.tp_op >= 0) {
      w.q_op = take(Nz * L * p->D * u);
      w.gm_op = take(Nz * p->D * size_t(std::max(c.num_scalar, c.latent_mlp_width)));
      if (p->pipe.op_proj) w.dx2s_op = take(Nz * p->D * u);
    }
  }
  w.total = o;
  return w;
}

extern "C" size_t aa_model_workspace_bytes(const aa_model_plan* plan, int64_t N, int64_t E, int with_forces) {
  if (!plan) return 0;
  return layout_workspace(plan, N, E, with_forces).total;
}

// Blocked step (aa_model_energy_forces_blocked): ONE arena -- the layout above at the edge count of the largest block, used by one
// block after the other -- followed by the frame part: the rebased row pointers of the block in flight [N+1], the flag of the cut
// check, and on a force step the two frame-wide [E,4] arrays every block writes its rows of.
struct BlockedWorkspace {
  Workspace arena;
  size_t rowptr, bad, vec, dvec, total;
};
static BlockedWorkspace layout_blocked(const aa_model_plan* p, int64_t N, int64_t E, int64_t max_block_edges, int with_forces) {
  BlockedWorkspace b{};
  b.arena = layout_workspace(p, N, max_block_edges, with_forces);
  size_t o = b.arena.total;
  auto take = [&](size_t bytes) {
    size_t r = o;
    o += (bytes + 255) / 256 * 256;
    return r;
  };
  b.rowptr = take(sizeof(int32_t) * (size_t(N) + 1));
  b.bad = take(sizeof(int32_t));
  if (with_forces) {
    b.vec = take(size_t(E) * 4 * p->esize());
    b.dvec = take(size_t(E) * 4 * p->esize());
  }
  b.total = o;
  return b;
}

extern "C" size_t aa_model_blocked_workspace_bytes(const aa_model_plan* plan, int64_t N, int64_t E, int64_t max_block_edges, int with_forces) {
  if (!plan || N < 0 || E < 0 || max_block_edges < 0) return 0;
  return layout_blocked(plan, N, E, std::min(max_block_edges, E), with_forces).total;
}

// ------------------------------------------------------------------------------------------------
// pipeline
// ------------------------------------------------------------------------------------------------
namespace {

inline Seg seg(void* p, int ld, int n) { return Seg{p, ld, n}; }

// optional per-stage timing with HIP events recorded on the launch stream
struct StageProfile {
  std::vector<std::string> names;
  std::vector<hipEvent_t> events;
  std::vector<double> bytes, flops;  // algorithmic HBM bytes / flops of the launch that ended at this mark
  int mark(const char* name, hipStream_t s, double by, double fl) {
    hipEvent_t e;
    AA_CHECK_HIP(hipEventCreate(&e));
    AA_CHECK_HIP(hipEventRecord(e, s));
    names.emplace_back(name);
    events.push_back(e);
    bytes.push_back(by);
    flops.push_back(fl);
    return AA_OK;
  }
  void clear() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    events.clear();
    names.clear();
    bytes.clear();
    flops.clear();
  }
};

template <typename T>
struct Runner {
  const aa_model_plan* p;
  const T* wts;
  char* ws;
  Workspace w;
  int64_t E, N;
  hipStream_t stream;
  StageProfile* prof = nullptr;
  StepPlan sp{};  // the launches of this step (choose_step): set by run_model, read everywhere below
  void* e_out = nullptr;  // atom_energy of this step (what the pair potential adds to)
  // one block of a blocked force step (StepPlan::block): the [E,4] rows of vec / dvec are those of the frame-wide arrays (the workspace
  // slots of the same name stay unused)
  void* frame_vec = nullptr;
  void* frame_dvec = nullptr;
  T* vec_rows() const { return frame_vec ? static_cast<T*>(frame_vec) : buf(w.vec); }
  T* dvec_rows() const { return frame_dvec ? static_cast<T*>(frame_dvec) : buf(w.dvec); }

  // per_edge / per_atom: operand elements the launch must move (each distinct operand row once); see DESIGN.md §5
  int mark(const char* name, double per_edge = 0, double per_atom = 0, double flops = 0) {
    return prof ? prof->mark(name, stream, sizeof(T) * (per_edge * double(E) + per_atom * double(N)), flops) : AA_OK;
  }
  static double seg_elems(const SegList& s) {
    double n = 0;
    for (int i = 0; i < s.count; ++i)
      if (s.s[i].p) n += s.s[i].n;
    return n;
  }
  // A read + C written (+ accumulated segments re-read) + Z + add operands of one GEMM, elements per row
  static double gemm_row_elems(const GemmArgs& g, bool a_from_hbm) {
    double n = (a_from_hbm ? seg_elems(g.a) : 0) + seg_elems(g.c);
    for (int i = 0; i < g.c.count; ++i)
      if (g.c.s[i].p && g.c_accum[i]) n += g.c.s[i].n;
    if (g.has_z) n += seg_elems(g.z);
    if (g.has_add) n += seg_elems(g.add);
    return n;
  }

  T* buf(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  const T* wt(size_t off) const { return wts + off; }

  // the plan's kernel-selection options of the linear layers
  void gemm_options(GemmArgs& g) const {
    g.force_kernel = p->opt.gemm_valu ? 3 : (p->opt.gemm_fp32_mfma ? 1 : 0);
    g.opt_v1 = p->opt.gemm_v1;
    g.opt_lds_epilogue = p->opt.gemm_lds_epilogue;
    g.opt_f64_column_loop = p->opt.f64_column_loop;
    g.opt_f64_rows = p->opt.f64_rows;
  }
  int gemm(const SegList& a, int act_a, const GemmMat& m, const SegList& c, const SegList* z = nullptr, const SegList* add = nullptr, int act_lo = 0,
           int act_hi = 0) {
    return gemm(a, act_a, wt(m.w), wt(m.wp), wt(m.wq), m.K, m.N, c, nullptr, z, add, act_lo, act_hi);
  }
  int gemm(const SegList& a, int act_a, const T* B, const T* Bp, const T* Bq, int K, int Nn, const SegList& c,
           const int* accum, const SegList* z, const SegList* add = nullptr, int act_lo = 0, int act_hi = 0) {
    GemmArgs g{};
    g.act_lo = act_lo;
    g.act_hi = act_hi;
    g.M = E;
    g.K = K;
    g.N = Nn;
    g.a = a;
    g.B = B;
    g.Bp = Bp;
    g.Bq = sizeof(T) == 4 ? Bq : nullptr;
    g.c = c;
    for (int i = 0; i < 3; ++i) g.c_accum[i] = accum ? accum[i] : 0;
    g.has_z = z ? 1 : 0;
    if (z) g.z = *z;
    g.act_a = act_a;
    g.act_kind = act_now;
    gemm_options(g);
    g.has_add = add ? 1 : 0;
    if (add) g.add = *add;
    if (int rc = launch_gemm<T>(g, stream)) return rc;
    if (!prof) return AA_OK;
    char nm[32];
    snprintf(nm, sizeof(nm), "gemm_%dx%d", K, Nn);
    return mark(nm, gemm_row_elems(g, true), 0, 2.0 * double(E) * K * Nn);
  }

  int act_now = AA_ACT_SILU;  // nonlinearity of the MLP whose layers are being launched (gemm() reads it)
  // forward of a ScalarMLPFunction: hidden pre-activations to h[i]; final linear output to `out`
  // which: 0 scalar_embed_mlp, 1 latent, 2 readout (selects the nonlinearity)
  int mlp_fwd(const MlpLayout& m, int nlayers, const SegList& in, const size_t* h, const SegList& out, int which) {
    act_now = p->cfg.act_kind[which];
    SegList a = in;
    for (int i = 0; i < nlayers; ++i) {
      SegList c;
      if (i < nlayers - 1) {
        c.count = 1;
        c.s[0] = seg(buf(h[i]), m.dims[i + 1], m.dims[i + 1]);
      } else {
        c = out;
      }
      if (int rc = gemm(a, i > 0, wt(m.w[i]), wt(m.wp[i]), wt(m.wq[i]), m.dims[i], m.dims[i + 1], c, nullptr, nullptr)) return rc;
      a = c;
    }
    return AA_OK;
  }

  // reverse: g_out (grad of final output) -> g_in (with per-segment accumulate flags)
  // add_last: optional extra gradient wrt the ACTIVATED last hidden layer (moments path), added before silu'
  int mlp_bwd(const MlpLayout& m, int nlayers, const SegList& g_out, const size_t* h, const size_t* g_h,
              const SegList& g_in, const int* g_in_accum, int which, const SegList* add_last = nullptr) {
    act_now = p->cfg.act_kind[which];
    SegList a = g_out;
    for (int i = nlayers - 1; i >= 0; --i) {
      SegList c, z;
      const int* acc = nullptr;
      const SegList* zp = nullptr;
      if (i > 0) {
        c.count = 1;
        c.s[0] = seg(buf(g_h[i - 1]), m.dims[i], m.dims[i]);
        z.count = 1;
        z.s[0] = seg(buf(h[i - 1]), m.dims[i], m.dims[i]);
        zp = &z;
      } else {
        c = g_in;
        acc = g_in_accum;
      }
      const SegList* addp = (add_last && i == nlayers - 1 && i > 0) ? add_last : nullptr;
      if (int rc = gemm(a, 0, wt(m.wt[i]), wt(m.wtp[i]), wt(m.wtq[i]), m.dims[i + 1], m.dims[i], c, acc, zp, addp)) return rc;
      a = c;
    }
    return AA_OK;
  }

  EdgeGeomArgs geom(const aa_graph* g, const void* pos) const {
    const aa_model_config& c = p->cfg;
    EdgeGeomArgs a{};
    a.E = E;
    a.N = N;
    a.center = g->center;
    a.nbr = g->nbr;
    a.types = g->types;
    a.pos = pos;
    a.shift_vec = g->shift_vec;
    a.num_types = c.num_types;
    a.num_bessels = c.num_bessels;
    a.l_max = c.l_max;
    a.S0 = c.embed_dim;
    a.poly_p = c.poly_p;
    a.rmax_recip = wt(p->blob.o_rmax);
    a.bessel_w = wt(p->blob.o_bessel);
    a.center_embed = wt(p->blob.o_cemb);
    a.neighbor_embed = wt(p->blob.o_nemb);
    a.basis_w = wt(p->blob.o_basis);
    a.embed_kind = c.embed_kind;
    a.spline_span = c.spline_span;
    a.emb_tab = p->pipe.two_body_table ? wt(p->blob.o_embtab) : nullptr;
    a.vec = vec_rows();
    a.sh = buf(w.sh);
    a.emb0 = buf(w.emb0);
    return a;
  }

  ReadoutArgs readout_args(const aa_graph* g, void* atom_energy) const {
    const aa_model_config& c = p->cfg;
    ReadoutArgs r{};
    r.E = E;
    r.N = N;
    r.rowptr = g->rowptr;
    r.center = g->center;
    r.types = g->types;
    if (c.readout_mlp_depth > 0) {
      r.h = buf(w.ro_h[c.readout_mlp_depth - 1]);
      r.ld = c.readout_mlp_width;
      r.H = c.readout_mlp_width;
      r.act = 1;
    } else {
      r.h = buf(w.fcat);
      r.ld = p->SL1;
      r.H = p->SL1;
      r.act = 0;
    }
    r.w = wt(p->blob.o_ro_last);
    r.act_kind = c.act_kind[2];
    r.factor = 1.0 / std::sqrt(2.0 * c.avg_num_neighbors);
    r.scales = c.has_scales ? wt(p->blob.o_scales) : nullptr;
    r.shifts = c.has_shifts ? wt(p->blob.o_shifts) : nullptr;
    r.atom_energy = atom_energy;
    r.edge_sum = (p->pipe.chains() && atom_energy) ? buf(w.e_edge) : nullptr;  // written by the forward readout chain
    return r;
  }

  // owned-block hint of the graph (per-atom kernels of the fast paths only visit these atoms)
  int64_t atom_begin(const aa_graph* g) const { return g->atom_end > g->atom_begin ? g->atom_begin : 0; }
  int64_t atom_end(const aa_graph* g) const { return g->atom_end > g->atom_begin ? g->atom_end : N; }

  TpChainArgs chain_args(const aa_graph* g) const {
    const aa_model_config& c = p->cfg;
    TpChainArgs a{};
    a.E = E;
    a.N = N;
    a.rowptr = g->rowptr;
    a.u = c.num_tensor;
    a.sh = buf(w.sh);
    a.ld_sh = p->D;
    a.w0 = buf(w.w0);
    a.ld_w0 = p->W;
    a.wenv0 = buf(w.envw[0]);
    a.ld_we0 = p->W;
    a.wenv1 = buf(w.envw[1]);
    a.ld_we1 = p->W;
    a.weights0 = wt(p->blob.o_tpw[0]);
    a.weights1 = wt(p->blob.o_tpw[1]);
    a.coupling = c.tps[0].coupling;
    a.sf = 1.0 / std::sqrt(c.avg_num_neighbors);
    a.x2s0 = buf(w.x2s[0]);
    a.x2s1 = buf(w.x2s[1]);
    a.scal1 = buf(w.scal[1]);
    a.ld_scal = c.num_tensor;
    a.ld_gscal = c.num_tensor;
    a.ld_gw0 = p->W;
    a.ld_gwe = p->W;
    a.ld_gsh = p->D;
    return a;
  }

  // ---- fused GEMM chains (LinearPath::Chains) -------------------------------------------------------------
  static ChainLayer chain_layer(int64_t M, const SegList& a, int act_a, const void* Bq, int K, int Nn, const SegList& c,
                                const int* accum, const SegList* z, const SegList* add, int use_prev, int keep_tile,
                                int keep_act) {
    ChainLayer L{};
    L.g.M = M;
    L.g.K = K;
    L.g.N = Nn;
    L.g.a = a;
    L.g.Bq = Bq;
    L.g.c = c;
    for (int i = 0; i < 3; ++i) L.g.c_accum[i] = accum ? accum[i] : 0;
    L.g.has_z = z ? 1 : 0;
    if (z) L.g.z = *z;
    L.g.has_add = add ? 1 : 0;
    if (add) L.g.add = *add;
    L.g.act_a = act_a;
    L.use_prev = use_prev;
    L.keep_tile = keep_tile;
    L.keep_act = keep_act;
    return L;
  }
  int run_chain(ChainArgs& ca, const char* tag) {
    ca.M = E;
    if (int rc = launch_gemm_chain(ca, stream)) return rc;
    if (!prof) return AA_OK;
    char nm[32];
    int o = snprintf(nm, sizeof(nm), "gc");
    double elems = 0, fl = 0, per_atom = 0;
    for (int i = 0; i < ca.nlayers; ++i) {
      if (o < 28) o += snprintf(nm + o, sizeof(nm) - o, "_%dx%d", ca.L[i].g.K, ca.L[i].g.N);
      elems += gemm_row_elems(ca.L[i].g, true);  // a is an empty list for use_prev layers (kept tile in registers)
      if (ca.L[i].a_mode == 2) elems += 2.0 * ca.L[i].g.a.s[0].n;  // (+ the add and z rows of the operand transform)
      fl += 2.0 * double(E) * ca.L[i].g.K * ca.L[i].g.N;
      if (ca.L[i].mom_gm0) {  // moments epilogue: + h, Y and d Y rows, the GM0 block of every atom once, two rank-D updates per row
        elems += 64 + 2.0 * ca.L[i].mom_d;
        per_atom += 64.0 * ca.L[i].mom_d;
        fl += 4.0 * double(E) * ca.L[i].mom_d * 64;
      }
    }
    (void)tag;
    return mark(nm, elems, per_atom, fl);
  }

  TpMomArgs mom_args(const aa_graph* g) const {
    const aa_model_config& c = p->cfg;
    TpMomArgs m{};
    m.c = chain_args(g);
    m.c.atom0 = atom_begin(g);
    m.c.N = atom_end(g);
    m.c.wenv0 = m.c.wenv1 = nullptr;
    m.a0 = buf(w.emb);
    m.ld_a0 = c.num_scalar;
    m.ka0 = c.num_scalar;
    m.a1 = buf(w.lat_h[0][c.latent_mlp_depth - 1]);
    m.ld_a1 = c.latent_mlp_width;
    m.ka1 = c.latent_mlp_width;
    m.wk0 = wt(p->blob.o_wk[0]);
    m.wt0 = wt(p->blob.o_wt[0]);
    m.wk1 = wt(p->blob.o_wk[1]);
    m.wt1 = wt(p->blob.o_wt[1]);
    m.waves_per_block = p->opt.moments_waves_per_block;
    return m;
  }

  TpOpArgs op_args(const aa_graph* g, int l) const {
    const aa_model_config& c = p->cfg;
    TpOpArgs o{};
    o.N = atom_end(g);
    o.atom0 = atom_begin(g);
    o.E = E;
    o.rowptr = g->rowptr;
    o.u = c.num_tensor;
    o.sh = buf(w.sh);
    o.ld_sh = p->D;
    o.w0 = buf(w.w0);
    o.ld_w0 = p->W;
    o.coupling = c.tps[0].coupling;
    o.sf = 1.0 / std::sqrt(c.avg_num_neighbors);
    for (int m = 0; m < c.num_layers && m < 3; ++m) {
      o.x2s[m] = buf(w.x2s[m]);
      o.tpw[m] = wt(p->blob.o_tpw[m]);
    }
    if (l == 0) {
      o.a = buf(w.emb);
      o.ld_a = o.ka = c.num_scalar;
      o.act = 0;
    } else {
      o.a = buf(w.lat_h[l - 1][c.latent_mlp_depth - 1]);
      o.ld_a = o.ka = c.latent_mlp_width;
      o.act = 1;
    }
    o.wk = wt(p->blob.o_wk[l]);
    o.wt = wt(p->blob.o_wt[l]);
    if (sp.slot) {
      // env inputs are hidden pre-activations everywhere: scalar_embed_mlp's (env weights behind its output layer) for layer 0,
      // slot l of the dense-net buffer (= z_{l-1}) afterwards
      if (l == 0) {
        o.a = buf(w.se_h[c.embed_mlp_depth - 1]);
        o.ld_a = o.ka = c.embed_mlp_width;
        o.act = 1;
        o.wk = wt(p->blob.o_s_wk0);
        o.wt = wt(p->blob.o_s_wt0);
      } else {
        o.a = buf(w.fcat) + size_t(c.num_scalar) * l;
        o.ld_a = p->SL1;
      }
    }
    o.ld_scal = c.num_tensor;
    o.ld_gscal = c.num_tensor;
    o.q = buf(w.q_op);
    o.num_layers = c.num_layers;
    o.bvec = sp.op_split ? buf(w.bvec_op) : nullptr;
    o.gmbuf = sp.op_split_reverse ? buf(w.gm_op) : nullptr;
    o.mbuf = sp.op_split ? buf(w.mom_op) : nullptr;
    o.ld_gw0 = p->W;
    o.ld_gsh = p->D;
    o.ka_lds = std::max(c.num_scalar, c.latent_mlp_width);
    o.env_mfma = (sizeof(T) == 8 && !p->opt.op_env_vector && (o.ld_a % 2) == 0) ? 1 : 0;
    return o;
  }

  // one problem per spherical-harmonic component j (rows: atoms), weight matrix number r(j)
  int proj_gemm(const TpOpArgs& o, const GemmMatSet& ms, const T* a_base, int64_t a_ld, int64_t a_bs, T* c_base, int64_t c_ld, int64_t c_bs) {
    GemmArgs gm{};
    gm.M = o.N - o.atom0;
    gm.K = ms.K;
    gm.N = ms.N;
    gm.a = SegList{1, {seg(const_cast<T*>(a_base) + o.atom0 * a_ld, int(a_ld), ms.K)}};
    gm.c = SegList{1, {seg(c_base + o.atom0 * c_ld, int(c_ld), ms.N)}};
    gm.B = wt(ms.w);
    gm.Bp = wt(ms.wp);
    gm.Bq = sizeof(T) == 4 ? wt(ms.wq) : nullptr;
    gm.act_kind = AA_ACT_SILU;
    gemm_options(gm);
    gm.batch = p->D;
    gm.a_bs = a_bs;
    gm.c_bs = c_bs;
    gm.b_bs = int64_t(ms.w_bs);
    gm.bp_bs = int64_t(ms.wp_bs);
    gm.bq_bs = int64_t(ms.wq_bs);
    for (int j = 0, r = 0; j < p->D; ++j) {
      if (j >= (r + 1) * (r + 1)) ++r;
      gm.bsel4 |= static_cast<unsigned long long>(r) << (4 * j);
    }
    if (int rc = launch_gemm<T>(gm, stream)) return rc;
    return mark("op_proj_gemm", 0, double(p->D) * (ms.K + ms.N), 2.0 * double(gm.M) * p->D * ms.K * ms.N);
  }
  // forward of tensor-product layer l on the operator kernels
  int run_op_fwd(const aa_graph* g, int l) {
    const int u = p->cfg.num_tensor;
    TpOpArgs o = op_args(g, l);
    o.scal = buf(w.scal[l]);
    if (sp.proj_forward) {
      o.proj_gemm = 1;
      if (int rc = launch_tp_op<T>(p->pipe.tp_op, l, false, o, stream, 1)) return rc;
      if (int rc = mark("tp_op_moments", p->D + o.ka)) return rc;
      const GemmMatSet& ms = (l == 0 && sp.slot) ? p->blob.s_pr0f : p->blob.s_pr[l];
      if (int rc = proj_gemm(o, ms, buf(w.mom_op), int64_t(p->D) * o.ka, o.ka, buf(w.x2s[l]), int64_t(p->D) * u, u)) return rc;
      if (int rc = launch_tp_op<T>(p->pipe.tp_op, l, false, o, stream, 2)) return rc;
      return mark("tp_op_fwd", p->W + u, double(l + 1) * p->D * u);
    }
    if (int rc = launch_tp_op<T>(p->pipe.tp_op, l, false, o, stream)) return rc;
    return mark("tp_op_fwd", p->D + o.ka + p->W + u, double(l + 1) * p->D * u);
  }
  // reverse of tensor-product layer l on the operator kernels: d scal_m -> d w0 / d Y (layer 0), d (env input) -> g_aenv
  int run_op_bwd(const aa_graph* g, int l) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, W = p->W;
    TpOpArgs o = op_args(g, l);
    for (int m = 0; m < L; ++m) o.gscal[m] = buf(w.g_scal[m]);
    o.g_w0 = buf(w.g_w0);
    o.gsh_x1 = buf(w.g_sh);
    size_t slot = size_t(u / 64);
    for (int m = 0; m < l; ++m) slot += size_t(m == 0 ? S : c.latent_mlp_width) / 64;
    o.gsh_env = buf(w.g_sh) + slot * size_t(E) * p->D;
    o.g_a = buf(w.g_aenv);
    o.ld_ga = o.ka;
    // (split form: every forward kernel of this step stored its B_l next to the others -- the vectors the layer-0 reverse needs)
    o.bvec_ready = (o.bvec && !p->opt.op_recompute_bvecs) ? 1 : 0;
    const double elems = p->D + W + u + 2 * o.ka + p->D + (l == 0 ? W + double(L - 1) * u + p->D : 0);
    if (sp.proj_reverse) {
      o.proj_gemm = 1;
      o.dx2s = buf(w.dx2s_op);
      if (int rc = launch_tp_op<T>(p->pipe.tp_op, l, true, o, stream, 1)) return rc;
      if (int rc = mark("tp_op_bwd", elems - 2 * o.ka - p->D, double(L) * p->D * u)) return rc;
      const GemmMatSet& ms = (l == 0 && sp.slot) ? p->blob.s_prt0f : p->blob.s_prt[l];
      if (int rc = proj_gemm(o, ms, buf(w.dx2s_op), int64_t(p->D) * u, u, buf(w.gm_op), int64_t(p->D) * o.ka, o.ka)) return rc;
      if (int rc = launch_tp_op<T>(p->pipe.tp_op, l, true, o, stream, 2)) return rc;
      return mark("tp_op_edge_env", 2 * o.ka + p->D);
    }
    if (int rc = launch_tp_op<T>(p->pipe.tp_op, l, true, o, stream)) return rc;
    return mark("tp_op_bwd", elems, double(L) * p->D * u);
  }

  TpOperand implicit(size_t w_off) const {
    TpOperand o{};
    o.sh = buf(w.sh);
    o.ld_sh = p->D;
    o.w = buf(w_off);
    o.ldw = p->W;
    return o;
  }

  // ---- the whole forward in one launch (aa_fused.hip; StepPlan::forward says when) -------------------------------------

  // everything but the weight program
  FusedFwdArgs fused_args(const aa_graph* g, const void* pos, void* atom_energy) const {
    const aa_model_config& c = p->cfg;
    FusedFwdArgs a{};
    a.N = N;
    a.atom0 = atom_begin(g);
    a.atom_end = atom_end(g);
    a.rowptr = g->rowptr;
    a.nbr = g->nbr;
    a.types = g->types;
    a.pos = static_cast<const float*>(pos);
    a.shift_vec = static_cast<const float*>(g->shift_vec);
    // segments of more than one 32-edge tile: teams of waves, dealt from class lists in the workspace
    a.tile_atoms = nullptr;
    a.tile_counts = nullptr;
    a.tile_cap = 0;
    if (sp.forward != ForwardKind::FusedOneTile) {
      a.tile_counts = reinterpret_cast<int32_t*>(buf(w.tiles));
      a.tile_atoms = a.tile_counts + 8;
      a.tile_cap = g->num_atoms;
      a.mixed = sp.forward == ForwardKind::FusedMixed ? 1 : 0;
    }
    a.num_types = c.num_types;
    a.embed_kind = c.embed_kind;
    a.spline_span = c.spline_span;
    a.poly_p = float(c.poly_p);
    a.rmax_recip = wf(p->blob.o_rmax);
    a.bessel_w = wf(p->blob.o_bessel);
    a.emb_tab = wf(p->blob.o_embtab_h);  // (folded: the table yields the first layer's pre-activation)
    a.tpw0 = wf(p->blob.o_tpw[0]);
    a.tpw1 = wf(p->blob.o_tpw[1]);
    a.coupling = c.tps[0].coupling;
    a.sf = float(1.0 / std::sqrt(c.avg_num_neighbors));
    a.ro_w = wf(p->blob.o_ro_last);
    a.ro_factor = float(1.0 / std::sqrt(2.0 * c.avg_num_neighbors));
    a.scales = c.has_scales ? wf(p->blob.o_scales) : nullptr;
    a.shifts = c.has_shifts ? wf(p->blob.o_shifts) : nullptr;
    a.vec = reinterpret_cast<float*>(vec_rows());
    a.sh = bf(w.sh);
    a.se_h = bf(w.se_h[0]);
    a.emb = bf(w.emb);
    a.w0 = bf(w.w0);
    a.lat_h0 = bf(w.lat_h[0][0]);
    a.lat_h1 = bf(w.lat_h[1][0]);
    a.ro_h = bf(w.ro_h[0]);
    a.fcat = nullptr;
    a.x2s0 = bf(w.x2s[0]);
    a.x2s1 = bf(w.x2s[1]);
    a.atom_energy = static_cast<float*>(atom_energy);
    a.status = p->status;
    a.fill_done = sp.block ? 1 : 0;  // (a block leaves the energies of the other blocks' atoms alone)
    return a;
  }
  const float* wf(size_t off) const { return reinterpret_cast<const float*>(wt(off)); }
  float* bf(size_t off) const { return reinterpret_cast<float*>(buf(off)); }

  // the weight program of a fused-forward kernel under construction (see fused_fwd_kernel): 12-KB blocks in execution order
  struct FusedProgram {
    FusedFwdArgs& a;
    int R;
    int ns = 0;
    void layer(const float* Wq, int KC, int tile0, int ntiles) {
      for (int t = tile0; t < tile0 + ntiles; t += 2)
        for (int kc = 0; kc < KC; ++kc) step(Wq + (size_t(t) * KC + kc) * 64 * 24, Wq + (size_t(t + 1) * KC + kc) * 64 * 24);
    }
    void chunk(const float* Wq, int KC, int kc) { step(Wq + size_t(kc) * 64 * 24, Wq + (size_t(KC) + kc) * 64 * 24); }  // the tile pair (0, 1) x chunk kc of a KC-chunk layer
    void env(const float* Wk) {  // one env projection: 4 blocks of env-weight rows
      for (int cblk = 0; cblk < 4; ++cblk) rows(Wk + size_t(cblk) * 16 * R * 64);
    }
    void rows(const float* W) { step(W, W + 1536); }  // (blocks are loaded as 2 x 6 KB; 16 R 256 B are used)
    void step(const float* lo, const float* hi) {
      if (ns < kFusedMaxSteps) {
        a.wstep[ns][0] = lo;
        a.wstep[ns][1] = hi;
      }
      ++ns;
    }
  };

  // the one-wave form's program.  The plan takes the fused forward only with every fold of its program packed (choose_pipeline:
  // fold_embed_table, fold_embed_output, fold_latent_outputs)
  int fused_program_one_wave(FusedFwdArgs& a) const {
    FusedProgram prog{a, p->R};
    prog.env(wf(p->blob.o_wk0f));
    prog.layer(wf(p->blob.o_g0fq), 2, 0, 2 + 2 * p->R);
    prog.layer(wf(p->blob.latent[0].wq[0]), 4, 0, 2);
    prog.env(wf(p->blob.o_wk[1]));
    prog.layer(wf(p->blob.o_lat1in_fq), 6, 0, 2);
    prog.layer(wf(p->blob.o_ro0_fq), 6, 0, 2);
    if (prog.ns != fused_fwd_num_steps(p->R) || prog.ns > kFusedMaxSteps) return fail(AA_ERR_INVALID, "fused forward: program length mismatch");
    return AA_OK;
  }

  // the program of the two-waves-per-SIMD forms of the one-tile pass (aa_fused8.hip): their own step order -- Wenv0 | first stage |
  // latent 0 | Wenv1 | latent 1: scal1 chunks | [lat0, two-body] chunks x {latent 1, readout} | readout: lat1 chunks [| readout-reverse
  // chain [| deep tail]] -- and what the tail writes
  int fused_program_wide(FusedFwdArgs& a8, ReverseInForward tail) const {
    FusedProgram prog{a8, p->R};
    prog.env(wf(p->blob.o_wk0f));
    prog.layer(wf(p->blob.o_g0fq), 2, 0, 2 + 2 * p->R);
    prog.layer(wf(p->blob.latent[0].wq[0]), 4, 0, 2);
    prog.env(wf(p->blob.o_wk[1]));
    prog.chunk(wf(p->blob.o_lat1in_fq), 6, 4);
    prog.chunk(wf(p->blob.o_lat1in_fq), 6, 5);
    for (int kc : {2, 3, 0, 1}) {
      prog.chunk(wf(p->blob.o_lat1in_fq), 6, kc);
      prog.chunk(wf(p->blob.o_ro0_fq), 6, kc);
    }
    prog.chunk(wf(p->blob.o_ro0_fq), 6, 4);
    prog.chunk(wf(p->blob.o_ro0_fq), 6, 5);
    if (tail != ReverseInForward::None) {
      prog.layer(wf(p->blob.o_b3af_q), 2, 0, 2);
      prog.layer(wf(p->pipe.fold_lat0_reverse ? p->blob.o_b3bf_q : p->blob.o_b3b_q), 4, 0, 4);
      prog.layer(wf(p->blob.o_b3c_q), 2, 0, 2);
      a8.g_fcat = bf(w.g_fcat);
      a8.ld_gfcat = p->SL1;
      a8.g_scal1 = bf(w.g_scal[1]);
    }
    if (tail == ReverseInForward::ChainMomentsLatent0) {
      // + the transposed layer-1 env weights [R][u][64] as they are packed for tp_mom_bwd_last -- four windows of 48 of their
      //   64 R rows, the last one(s) pulled back inside the matrix (fused_fwd8_kernel: project_moments_t) -- and the first
      //   layer of latent 0, transposed (the resident chain's bytes)
      for (int cblk = 0; cblk < 4; ++cblk) prog.rows(wf(p->blob.o_wt[1]) + size_t(std::min(48 * cblk, 64 * p->R - 48)) * 64);
      prog.layer(wf(p->blob.latent[0].wtq[0]), 2, 0, 4);
      a8.g_scal0 = bf(w.g_scal[0]);
      a8.gsh_env1 = bf(w.g_sh) + size_t(2) * size_t(E) * p->D;
    }
    if (prog.ns != fused_fwd8_num_steps(p->R, int(tail)) || prog.ns > kFusedMaxSteps) return fail(AA_ERR_INVALID, "fused forward (wide): program length mismatch");
    return AA_OK;
  }

  // algorithmic traffic: neighbor id + shift in; unit vector, harmonics, five 64-wide rows and w0 out per edge;
  // position, two x2s blocks, energy, row pointer per atom.  Flops: the linear layers of the forward (w0 counted once).
  int mark_fused_fwd(const aa_graph* g) {
    const int S = p->cfg.num_scalar, u = p->cfg.num_tensor;
    double per_edge = 1 + (g->shift_vec ? 3 : 0) + 3 + 4 + p->D + 5 * 64 + p->W;
    const double per_atom = 3 + 2.0 * p->D * u + 1 + 1;
    double fl = 2.0 * double(E) * (2.0 * 64 * 64 + 64.0 * p->blob.ng0 + double(S + u) * 64 + 64.0 * S + double(2 * S + u) * 64 + 64.0 * S + 3.0 * S * 64);
    if (sp.reverse_in_forward != ReverseInForward::None) {  // (+ the readout-reverse chain: 192 gradient columns out instead of two 64-wide pre-activation rows)
      fl += 2.0 * double(E) * (64.0 * 64 + 128.0 * 128 + 64.0 * 64);
      per_edge += 64;
    }
    if (sp.reverse_in_forward == ReverseInForward::ChainMomentsLatent0) {  // (+ the latent-0 reverse layer; out: d EDGE_FEATURES[:, :64], d scal0, d scal1, d Y instead of 192 columns; lat_h0 read again)
      fl += 2.0 * double(E) * 64.0 * 128;
      per_edge += 64 + p->D;
    }
    return mark("fused_fwd", per_edge, per_atom, fl);
  }

  int forward_fused(const aa_graph* g, const void* pos, void* atom_energy) {
    FusedFwdArgs a = fused_args(g, pos, atom_energy);
    if (int rc = fused_program_one_wave(a)) return rc;  // (the team pass of the mixed form runs it whatever the one-tile pass's form)
    if (sp.fused_form == FusedForm::OneWave) {
      if (int rc = mark("begin")) return rc;
      if (int rc = launch_fused_fwd(p->pipe.chain_pair, sp.fused_form, a, nullptr, stream)) return rc;
      return mark_fused_fwd(g);
    }
    FusedFwdArgs a8 = a;
    if (int rc = fused_program_wide(a8, fused_tail(sp.fused_form))) return rc;
    if (int rc = mark("begin")) return rc;
    if (int rc = launch_fused_fwd(p->pipe.chain_pair, sp.fused_form, a, &a8, stream)) return rc;
    return mark_fused_fwd(g);
  }

  // ---- staged forward, stage by stage ----------------------------------------------------------------------------------

  // 1-2: geometry, SH, radial-chemical embedding; 3: scalar_embed_mlp; 4+5a: env_embed_linear and
  // first_layer_env_embed_projection as ONE GEMM (tensorembed.py:89, _allegro.py:251)
  int fwd_first_stage(const aa_graph* g, const void* pos) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, W = p->W, SL1 = p->SL1;
    if (int rc = mark("begin")) return rc;
    const double idx2 = 8.0 / sizeof(T);  // center + nbr ids, in elements
    if (int rc = launch_edge_prologue<T>(geom(g, pos), stream)) return rc;
    if (int rc = mark("edge_prologue", idx2 + 6 + (g->shift_vec ? 3 : 0) + 4 + p->D + c.embed_dim)) return rc;
    SegList in{1, {seg(buf(w.emb0), c.embed_dim, c.embed_dim)}};
    if (p->pipe.chains()) {
      // 3 + 4 + 5a as ONE kernel: emb0 -> h_e -> emb -> [two_body | w0]; hidden layers stay in registers
      const SegList none{0, {}};
      ChainArgs ca{};
      SegList c0{1, {seg(buf(w.se_h[0]), 64, 64)}};
      SegList c1{1, {seg(buf(w.emb), S, S)}};
      SegList c2{2, {seg(buf(w.fcat), SL1, S), seg(buf(w.w0), W, W)}};
      ca.L[0] = chain_layer(E, in, 0, wt(p->blob.embed.wq[0]), c.embed_dim, 64, c0, nullptr, nullptr, nullptr, 0, 0, 1);
      if (sp.forward == ForwardKind::StagedFolded) {
        // folded: a_e = silu(h_e) is stored where the embedding used to be; [two_body | w0] = a_e @ (W1 G0)
        ca.nlayers = 2;
        ca.L[0].kept_out = buf(w.emb);
        ca.L[0].ld_kept = S;
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.o_g0fq), 64, p->blob.ng0, c2, nullptr, nullptr, nullptr, 1, -1, 0);
      } else {
        ca.nlayers = 3;
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.embed.wq[1]), 64, S, c1, nullptr, nullptr, nullptr, 1, 0, 0);
        ca.L[2] = chain_layer(E, none, 0, wt(p->blob.o_g0q), 64, p->blob.ng0, c2, nullptr, nullptr, nullptr, 1, -1, 0);
      }
      return run_chain(ca, "F1");
    }
    if (sp.slot) {
      // 3: hidden layers of scalar_embed_mlp; 4 + 5a on the activated last hidden layer (output layer folded into G0)
      const int De = c.embed_mlp_depth, He = c.embed_mlp_width;
      SegList hid{1, {seg(buf(w.se_h[De - 1]), He, He)}};
      if (int rc = mlp_fwd(p->blob.embed, De, in, w.se_h, hid, 0)) return rc;
      SegList out{2, {seg(buf(w.fcat), SL1, S), seg(buf(w.w0), W, W)}};
      act_now = c.act_kind[0];
      return gemm(hid, 1, p->blob.s_g0f, out);
    }
    SegList emb{1, {seg(buf(w.emb), S, S)}};
    if (int rc = mlp_fwd(p->blob.embed, c.embed_mlp_depth + 1, in, w.se_h, emb, 0)) return rc;
    SegList out{3, {seg(buf(w.fcat), SL1, S), seg(buf(w.w0), W, W), seg(buf(w.envw[0]), W, W)}};
    if (p->pipe.env_moments()) out.count = 2;
    act_now = AA_ACT_SILU;  // (a plain linear map: no activation involved)
    return gemm(emb, 0, wt(p->blob.o_g0), wt(p->blob.o_g0p), wt(p->blob.o_g0q), S, p->blob.ng0, out, nullptr, nullptr);
  }

  // operands both directions of a tensor-product layer take, per-edge kernels with compile-time tables (TpPath::Spec, SpecChain) ...
  template <typename A>
  void spec_operands(A& a, const aa_graph* g, int l) const {
    a.E = E;
    a.N = N;
    a.rowptr = g->rowptr;
    a.u = p->cfg.num_tensor;
    a.sh = buf(w.sh);
    a.ld_sh = p->D;
    if (l == 0) {
      a.w_x1 = buf(w.w0);
      a.ld_w1 = p->W;
    } else {
      a.x1_dense = buf(w.tf[l - 1]);
    }
    a.w_env = buf(w.envw[l]);
    a.ld_we = p->W;
    a.weights = wt(p->blob.o_tpw[l]);
    a.coupling = p->cfg.tps[l].coupling;
    a.sf = 1.0 / std::sqrt(p->cfg.avg_num_neighbors);
    a.x2s = buf(w.x2s[l]);
  }
  // ... and on LDS coupling tables (TpPath::General)
  template <typename A>
  void general_operands(A& a, const aa_graph* g, int l) const {
    a.E = E;
    a.N = N;
    a.rowptr = g->rowptr;
    if (l == 0)
      a.x1 = implicit(w.w0);
    else
      a.x1.dense = buf(w.tf[l - 1]);
    a.x2 = implicit(w.envw[l]);
    a.weights = wt(p->blob.o_tpw[l]);
    a.scatter_factor = 1.0 / std::sqrt(p->cfg.avg_num_neighbors);
    a.x2s = buf(w.x2s[l]);
  }

  // 5: tensor-product layer l
  int fwd_tp_layer(const aa_graph* g, int l) {
    const int u = p->cfg.num_tensor, L = p->cfg.num_layers, W = p->W;
    switch (p->pipe.tp) {
      case TpPath::Operator:
        return run_op_fwd(g, l);
      case TpPath::Moments: {
        TpMomArgs m = mom_args(g);
        if (l == 0) {
          m.c.scal1 = buf(w.scal[0]);  // the first-layer kernel writes its scalars through this field
          if (sp.forward == ForwardKind::StagedFolded) m.wk0 = wt(p->blob.o_wk0f);  // (its env input is a_e: env weights behind the output layer of scalar_embed_mlp)
          if (int rc = launch_tp_mom_fwd_first<T>(p->pipe.chain_pair, m, stream)) return rc;
          return mark("tp_mom_fwd_first", p->D + m.ka0 + W + u, double(p->D) * u);
        }
        if (int rc = launch_tp_mom_fwd_last<T>(p->pipe.chain_pair, m, stream)) return rc;
        return mark("tp_mom_fwd_last", p->D + m.ka1 + W + u, 2.0 * p->D * u);
      }
      case TpPath::SpecChain:
        if (l == 1) {
          if (int rc = launch_tp_chain_fwd_last<T>(p->pipe.chain_pair, chain_args(g), stream)) return rc;
          return mark("tp_chain_fwd_last", 2 * W + p->D + u, 2.0 * p->D * u);
        }
        [[fallthrough]];  // (layer 0 of the pair: the per-edge kernel, its [E,u,D] output not stored)
      case TpPath::Spec: {
        TpSpecFwdArgs a{};
        spec_operands(a, g, l);
        a.out = (l < L - 1 && p->pipe.chain_pair < 0) ? buf(w.tf[l]) : nullptr;
        a.scal = buf(w.scal[l]);
        a.ld_scal = u;
        if (int rc = launch_tp_spec_fwd<T>(p->pipe.spec_sig[l], a, stream)) return rc;
        return mark("tp_spec_fwd", 2 * W + p->D + u, 2.0 * p->D * u);
      }
      case TpPath::General: {
        TpLayerFwdArgs a{};
        general_operands(a, g, l);
        a.out = l < L - 1 ? buf(w.tf[l]) : nullptr;
        a.scal = buf(w.scal[l]);
        a.ld_scal = u;
        if (int rc = launch_tp_layer_fwd<T>(p->layers[l], a, stream)) return rc;
        return mark("tp_layer_fwd", 2 * W + p->D + u * p->D + u, 2.0 * p->D * u);
      }
    }
    return fail(AA_ERR_INVALID, "step plan: unknown tensor-product path");
  }

  // latent MLP l; on the chains the last one carries the readout's GEMM layer
  int fwd_latent(int l) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, W = p->W, SL1 = p->SL1;
    SegList in{2, {seg(buf(w.fcat), SL1, S * (l + 1)), seg(buf(w.scal[l]), u, u)}};
    if (p->pipe.chains()) {
      const SegList none{0, {}};
      const bool folded = sp.forward == ForwardKind::StagedFolded;
      ChainArgs ca{};
      SegList ch{1, {seg(buf(w.lat_h[l][0]), 64, 64)}};
      SegList cl{1, {seg(buf(w.fcat) + S * (l + 1), SL1, S)}};
      SegList fin{1, {seg(buf(w.fcat), SL1, S * L)}};
      SegList cr{1, {seg(buf(w.ro_h[0]), 64, 64)}};
      ca.L[0] = chain_layer(E, in, 0, wt(p->blob.latent[l].wq[0]), S * (l + 1) + u, 64, ch, nullptr, nullptr, nullptr, 0, 0, 1);
      if (folded && l < L - 1) {
        // folded: no output layer; a_l = silu(z_l) goes where lat_l used to be
        ca.nlayers = 1;
        ca.L[0].kept_out = buf(w.fcat) + S * (l + 1);
        ca.L[0].ld_kept = SL1;
      } else if (folded) {
        // folded: latent 1 and the readout on [two-body | a_0 | ...] with the output layers folded into their row blocks; a_1 stays in registers
        ca.nlayers = 2;
        ca.L[0] = chain_layer(E, in, 0, wt(p->blob.o_lat1in_fq), S * (l + 1) + u, 64, ch, nullptr, nullptr, nullptr, 0, 0, 1);
        ca.L[1] = chain_layer(E, fin, 0, wt(p->blob.o_ro0_fq), S * L + 64, 64, cr, nullptr, nullptr, nullptr, 1, -1, 0);
        ca.L[1].edge_sum_out = buf(w.e_edge);
        ca.ro_w = wt(p->blob.o_ro_last);
      } else if (l < L - 1) {
        ca.nlayers = 2;
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.latent[l].wq[1]), 64, S, cl, nullptr, nullptr, nullptr, 1, -1, 0);
      } else {
        // last latent + the readout's GEMM layer: lat_{L-1} stays in registers as the tail of the readout input
        ca.nlayers = 3;
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.latent[l].wq[1]), 64, S, cl, nullptr, nullptr, nullptr, 1, 0, 0);
        ca.L[2] = chain_layer(E, fin, 0, wt(p->blob.readout.wq[0]), S * L + 64, 64, cr, nullptr, nullptr, nullptr, 1, -1, 0);
        ca.L[2].edge_sum_out = buf(w.e_edge);  // last linear readout layer folded into the epilogue
        ca.ro_w = wt(p->blob.o_ro_last);
      }
      return run_chain(ca, "F2");
    }
    if (sp.slot) {
      // hidden pre-activation z_l straight into slot l + 1; the earlier slots are activated on load (their output layers are
      // folded into this layer's row blocks)
      SegList zl{1, {seg(buf(w.fcat) + S * (l + 1), SL1, S)}};
      act_now = c.act_kind[1];
      return gemm(in, l > 0, p->blob.s_in[l], zl, nullptr, nullptr, S, S * (l + 1));
    }
    SegList out;
    out.count = (l < L - 1 && !p->pipe.env_moments()) ? 2 : 1;
    out.s[0] = seg(buf(w.fcat) + S * (l + 1), SL1, S);
    if (l < L - 1 && !p->pipe.env_moments()) out.s[1] = seg(buf(w.envw[l + 1]), W, W);
    return mlp_fwd(p->blob.latent[l], c.latent_mlp_depth + 1, in, w.lat_h[l], out, 1);
  }

  // 6: edge readout GEMM layers (the chains ran theirs behind the last latent), 7-8: last linear + edge sum + per-type scale/shift
  int fwd_readout(const aa_graph* g, void* atom_energy) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, SL1 = p->SL1;
    if (c.readout_mlp_depth > 0 && !p->pipe.chains()) {
      act_now = c.act_kind[2];
      SegList a{1, {seg(buf(w.fcat), SL1, SL1)}};
      for (int i = 0; i < c.readout_mlp_depth; ++i) {
        SegList cs{1, {seg(buf(w.ro_h[i]), c.readout_mlp_width, c.readout_mlp_width)}};
        if (sp.slot && i == 0) {
          act_now = c.act_kind[1];  // (the activated columns are the latents' hidden layers)
          if (int rc = gemm(a, 1, p->blob.s_ro0, cs, nullptr, nullptr, S, SL1)) return rc;
          act_now = c.act_kind[2];
        } else if (int rc = gemm(a, i > 0, wt(p->blob.readout.w[i]), wt(p->blob.readout.wp[i]), wt(p->blob.readout.wq[i]), p->blob.readout.dims[i], p->blob.readout.dims[i + 1], cs,
                                 nullptr, nullptr)) {
          return rc;
        }
        a = cs;
      }
    }
    ReadoutArgs ra = readout_args(g, atom_energy);
    if (sp.block) {
      ra.atom0 = atom_begin(g);
      ra.N = atom_end(g);
    }
    if (sp.readout_grad_in_reduce) ra.g_h = buf(w.g_ro_h[c.readout_mlp_depth - 1]);
    if (int rc = launch_readout_reduce<T>(ra, stream)) return rc;
    return mark("readout_reduce", (p->pipe.chains() ? 1 : (c.readout_mlp_depth > 0 ? c.readout_mlp_width : SL1)) * (sp.readout_grad_in_reduce ? 2.0 : 1.0), 1);
  }

  int forward(const aa_graph* g, const void* pos, void* atom_energy) {
    if (sp.fused()) return forward_fused(g, pos, atom_energy);
    if (int rc = fwd_first_stage(g, pos)) return rc;
    for (int l = 0; l < p->cfg.num_layers; ++l) {
      if (int rc = fwd_tp_layer(g, l)) return rc;
      if (int rc = fwd_latent(l)) return rc;
    }
    return fwd_readout(g, atom_energy);
  }

  // ZBL pair potential (StepPlan::pair_zbl): adds to atom_energy, which the forward of this step has written, and -- on a force
  // step, behind edge_backward -- to the dvec rows (and to the forces where they are not gathered from dvec)
  int pair_zbl(const aa_graph* g, const void* pos, void* forces) {
    PairZblArgs a{};
    a.atom0 = atom_begin(g);
    a.atom_end = atom_end(g);
    a.rowptr = g->rowptr;
    a.nbr = g->nbr;
    a.types = g->types;
    a.pos = pos;
    a.shift_vec = g->shift_vec;
    a.num_types = p->cfg.num_types;
    a.rmax_recip = wt(p->blob.o_rmax);
    a.tab = p->zbl_tab;
    a.poly_p = p->zbl_poly_p;
    a.atom_energy = e_out;
    a.dvec = forces ? dvec_rows() : nullptr;
    a.forces = (forces && !sp.gather) ? forces : nullptr;
    if (int rc = launch_pair_zbl<T>(a, stream)) return rc;
    // per edge: neighbor index + its position and type (+ the shift vector), on a force step the dvec row read and written
    return mark("pair_zbl", 4.0 / sizeof(T) + 3 + 4.0 / sizeof(T) + (g->shift_vec ? 3 : 0) + (forces ? 8 : 0), 2 + 8.0 / sizeof(T));
  }

  // geometry reverse + force assembly (the end of every reverse pass)
  int edge_tail(const aa_graph* g, const void* pos, void* forces) {
    const aa_model_config& c = p->cfg;
    const int num_gsh = num_gsh_slots(p);
    EdgeBwdArgs eb{};
    eb.g = geom(g, pos);
    eb.g_emb0 = buf(w.g_emb0);
    eb.g_sh = buf(w.g_sh);
    eb.num_gsh = num_gsh;
    eb.forces = forces;
    if (p->pipe.embed_fused) eb.t_in = buf(w.trev);
    const bool gather = sp.gather;
    eb.dvec = dvec_rows();
    eb.gather = gather ? 1 : 0;
    if (int rc = launch_edge_backward<T>(eb, stream)) return rc;
    if (int rc = mark("edge_backward", 8.0 / sizeof(T) + 4 + (p->pipe.embed_fused ? c.num_bessels : c.embed_dim) + double(num_gsh) * p->D + (gather ? 4 : 6))) return rc;
    if (sp.pair_zbl)
      if (int rc = pair_zbl(g, pos, forces)) return rc;
    if (gather && !sp.block) {
      // deterministic force assembly: per atom, own segment minus transposed segment, fixed order (no atomics)
      ForceGatherArgs fg{N, g->rowptr, g->t_rowptr, g->t_perm, buf(w.dvec), forces};
      if (int rc = launch_force_gather<T>(fg, stream)) return rc;
      return mark("force_gather", 8.0 + 4.0 / sizeof(T), 3 + 8.0 / sizeof(T));
    }
    return AA_OK;
  }

  // Reverse pass of the slot form (LinearPath::Slot): per dense-net slot, top down.  Every layer here has a 128-wide (S)
  // output -- the accumulator-resident kernel's shape -- and writes its slot once.
  int backward_slot(const aa_graph* g, const void* pos, void* forces) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, W = p->W, SL1 = p->SL1;
    const int De = c.embed_mlp_depth, He = c.embed_mlp_width, Dr = c.readout_mlp_depth, Hr = c.readout_mlp_width, H = c.latent_mlp_width;
    if (sp.zero_forces) AA_CHECK_HIP(hipMemsetAsync(forces, 0, size_t(N) * 3 * sizeof(T), stream));
    if (int rc = mark("memset", 0, 3)) return rc;
    // readout: d (last hidden) from the energy, then its hidden layers down to the first one
    {
      ReadoutArgs r = readout_args(g, nullptr);
      r.g_h = buf(w.g_ro_h[Dr - 1]);
      act_now = c.act_kind[2];
      if (!sp.readout_grad_in_reduce) {
        if (int rc = launch_readout_backward<T>(r, stream)) return rc;
        if (int rc = mark("readout_backward", 2.0 * Hr)) return rc;
      }
      for (int i = Dr - 1; i >= 1; --i) {
        SegList a{1, {seg(buf(w.g_ro_h[i]), Hr, Hr)}};
        SegList cs{1, {seg(buf(w.g_ro_h[i - 1]), Hr, Hr)}};
        SegList z{1, {seg(buf(w.ro_h[i - 1]), Hr, Hr)}};
        if (int rc = gemm(a, 0, wt(p->blob.readout.wt[i]), wt(p->blob.readout.wtp[i]), wt(p->blob.readout.wtq[i]), p->blob.readout.dims[i + 1], p->blob.readout.dims[i], cs, nullptr, &z))
          return rc;
      }
    }
    for (int l = L - 1; l >= 0; --l) {
      // d z_l = ([d readout hidden | d z_{l+1} .. d z_{L-1}] @ stack_l + d a_l of the next layer's moments) * act'(z_l)
      SegList a{l < L - 1 ? 2 : 1, {seg(buf(w.g_ro_h[0]), Hr, Hr), seg(buf(w.g_fcat) + S * (l + 2), SL1, S * (L - 1 - l))}};
      SegList dz{1, {seg(buf(w.g_fcat) + S * (l + 1), SL1, S)}};
      SegList z{1, {seg(buf(w.fcat) + S * (l + 1), SL1, S)}};
      SegList ad{1, {seg(buf(w.g_aenv), H, H)}};
      act_now = c.act_kind[1];
      if (int rc = gemm(a, 0, p->blob.s_rs[l], dz, &z, l < L - 1 ? &ad : nullptr)) return rc;
      SegList gs{1, {seg(buf(w.g_scal[l]), u, u)}};
      if (int rc = gemm(dz, 0, p->blob.s_sct[l], gs)) return rc;
      // tensor-product layer reverse (per-atom operator kernels)
      if (int rc = run_op_bwd(g, l)) return rc;
    }
    // slot 0 (two-body scalars): every consumer's share in one layer
    {
      SegList a{2, {seg(buf(w.g_ro_h[0]), Hr, Hr), seg(buf(w.g_fcat) + S, SL1, S * L)}};
      SegList tb{1, {seg(buf(w.g_fcat), SL1, S)}};
      if (int rc = gemm(a, 0, p->blob.s_rstb, tb)) return rc;
    }
    // first stage + output layer of scalar_embed_mlp: d h = ([d two-body | d w0] @ (W_last G0)^T + d a_e of the moments) * act'(h)
    {
      SegList a{2, {seg(buf(w.g_fcat), SL1, S), seg(buf(w.g_w0), W, W)}};
      SegList dh{1, {seg(buf(w.g_se_h[De - 1]), He, He)}};
      SegList z{1, {seg(buf(w.se_h[De - 1]), He, He)}};
      SegList ad{1, {seg(buf(w.g_aenv), He, He)}};
      act_now = c.act_kind[0];
      if (int rc = gemm(a, 0, p->blob.s_g0ft, dh, &z, &ad)) return rc;
      SegList gi{1, {seg(buf(w.g_emb0), c.embed_dim, c.embed_dim)}};
      if (int rc = mlp_bwd(p->blob.embed, De, dh, w.se_h, w.g_se_h, gi, nullptr, 0)) return rc;
    }
    return edge_tail(g, pos, forces);
  }

  // ---- reverse pass, stage by stage (top down) ----------------------------------------------------------------------

  // zeroes what the reverse pass accumulates into (StepPlan::zero_gsh / zero_forces)
  int bwd_begin(void* forces) {
    const int num_gsh = num_gsh_slots(p);
    if (sp.zero_gsh) AA_CHECK_HIP(hipMemsetAsync(buf(w.g_sh), 0, size_t(E) * p->D * num_gsh * sizeof(T), stream));
    if (sp.zero_forces) AA_CHECK_HIP(hipMemsetAsync(forces, 0, size_t(N) * 3 * sizeof(T), stream));
    return mark("memset", sp.zero_gsh ? p->D * num_gsh : 0, 3);
  }

  // readout reverse; on the chains with the last latent's reverse in the same kernel
  int bwd_readout(const aa_graph* g) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, SL1 = p->SL1;
    if (p->pipe.chains()) {
      // (the fused forward of this step ran this chain in its tail: d EDGE_FEATURES[:, :S L] and d scal_{L-1} are in the workspace)
      if (sp.reverse_in_forward != ReverseInForward::None) return AA_OK;
      // readout reverse + last latent reverse in ONE kernel; d_lat_{L-1} and d_h never leave registers
      const SegList none{0, {}};
      ReadoutArgs r = readout_args(g, nullptr);
      ChainArgs ca{};
      ca.ro_w = r.w;
      ca.ro_factor = r.factor;
      ca.ro_scales = r.scales;
      ca.types = g->types;
      ca.center = g->center;
      SegList in{1, {seg(buf(w.ro_h[0]), 64, 64)}};
      // d_fcat[:, :S*L] receives the readout-reverse AND the latent-reverse contribution: instead of storing the
      // first and accumulating the second (write + read + write), the last layer takes both operands -- the
      // transformed readout hidden rows again (L2-resident) and the chained d_hidden -- against the stacked
      // weights [readout' ; latent'] and stores each tile once.
      SegList cn{1, {seg(nullptr, 64, 64)}};
      SegList z1{1, {seg(buf(w.lat_h[L - 1][0]), 64, 64)}};
      SegList c2{1, {seg(buf(w.g_fcat), SL1, S * L)}};
      SegList c3{1, {seg(buf(w.g_scal[L - 1]), u, u)}};
      if (p->pipe.fold_latent_outputs && L == 2) {
        // "d lat1 = d ro_h @ Wro[lat1]^T" and "d a1 = d lat1 @ Wout_1^T" as ONE 64x64 layer (folded at pack time): 12 instead of 14 steps
        ca.nlayers = 3;
        ca.L[0] = chain_layer(E, in, 0, wt(p->blob.o_b3af_q), 64, 64, cn, nullptr, &z1, nullptr, 0, 0, 0);
        ca.L[0].a_mode = 1;
        ca.L[1] = chain_layer(E, in, 0, wt(p->pipe.fold_lat0_reverse ? p->blob.o_b3bf_q : p->blob.o_b3b_q), 128, S * L, c2, nullptr, nullptr, nullptr, 1, -1, 0);
        ca.L[1].a_mode = 1;
        ca.L[2] = chain_layer(E, none, 0, wt(p->blob.o_b3c_q), 64, u, c3, nullptr, nullptr, nullptr, 1, -1, 0);
      } else {
        ca.nlayers = 4;
        ca.L[0] = chain_layer(E, in, 0, wt(p->blob.o_b3a_q), 64, S, cn, nullptr, nullptr, nullptr, 0, 0, 0);
        ca.L[0].a_mode = 1;
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.latent[L - 1].wtq[1]), S, 64, cn, nullptr, &z1, nullptr, 1, 0, 0);
        ca.L[2] = chain_layer(E, in, 0, wt(p->blob.o_b3b_q), 128, S * L, c2, nullptr, nullptr, nullptr, 1, -1, 0);
        ca.L[2].a_mode = 1;
        ca.L[3] = chain_layer(E, none, 0, wt(p->blob.o_b3c_q), 64, u, c3, nullptr, nullptr, nullptr, 1, -1, 0);
      }
      return run_chain(ca, "B3");
    }
    ReadoutArgs r = readout_args(g, nullptr);
    if (c.readout_mlp_depth == 0) {
      r.g_h = buf(w.g_fcat);
      if (int rc = launch_readout_backward<T>(r, stream)) return rc;
      return mark("readout_backward", 2.0 * SL1);
    }
    r.g_h = buf(w.g_ro_h[c.readout_mlp_depth - 1]);
    act_now = c.act_kind[2];
    if (!sp.readout_grad_in_reduce) {
      if (int rc = launch_readout_backward<T>(r, stream)) return rc;
      if (int rc = mark("readout_backward", 2.0 * c.readout_mlp_width)) return rc;
    }
    SegList a{1, {seg(r.g_h, c.readout_mlp_width, c.readout_mlp_width)}};
    for (int i = c.readout_mlp_depth - 1; i >= 0; --i) {
      SegList cs, z;
      const SegList* zp = nullptr;
      if (i > 0) {
        cs = SegList{1, {seg(buf(w.g_ro_h[i - 1]), c.readout_mlp_width, c.readout_mlp_width)}};
        z = SegList{1, {seg(buf(w.ro_h[i - 1]), c.readout_mlp_width, c.readout_mlp_width)}};
        zp = &z;
      } else {
        cs = SegList{1, {seg(buf(w.g_fcat), SL1, SL1)}};
      }
      if (int rc = gemm(a, 0, wt(p->blob.readout.wt[i]), wt(p->blob.readout.wtp[i]), wt(p->blob.readout.wtq[i]), p->blob.readout.dims[i + 1], p->blob.readout.dims[i], cs,
                        nullptr, zp))
        return rc;
      a = cs;
    }
    return AA_OK;
  }

  // reverse of latent MLP l
  int bwd_latent(int l) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, W = p->W, SL1 = p->SL1;
    if (p->pipe.chains() && l == L - 1) return AA_OK;  // (already done inside the readout chain)
    const SegList none{0, {}};
    ChainArgs ca{};
    SegList in{1, {seg(buf(w.g_fcat) + S * (l + 1), SL1, S)}};
    SegList c1{2, {seg(buf(w.g_fcat), SL1, S * (l + 1)), seg(buf(w.g_scal[l]), u, u)}};
    int acc1[3] = {1, 0, 0};
    switch (sp.latent_reverse) {
      case LatentReverse::Mlp: {
        SegList go;
        go.count = (l < L - 1 && !p->pipe.env_moments()) ? 2 : 1;
        go.s[0] = seg(buf(w.g_fcat) + S * (l + 1), SL1, S);
        if (l < L - 1 && !p->pipe.env_moments()) go.s[1] = seg(buf(w.g_envw), W, W);
        SegList aenv{1, {seg(p->pipe.env_moments() ? buf(w.g_aenv) : nullptr, c.latent_mlp_width, c.latent_mlp_width)}};
        const SegList* addp = (p->pipe.env_moments() && l < L - 1) ? &aenv : nullptr;
        return mlp_bwd(p->blob.latent[l], c.latent_mlp_depth + 1, go, w.lat_h[l], w.g_lat_h, c1, acc1, 1, addp);
      }
      case LatentReverse::InForwardTail:  // (ran in the deep tail of the fused forward)
        return AA_OK;
      case LatentReverse::TwoLayerChain: {
        ca.nlayers = 2;
        SegList cn{1, {seg(nullptr, 64, 64)}};
        SegList zz{1, {seg(buf(w.lat_h[l][0]), 64, 64)}};
        SegList ad{1, {seg(buf(w.g_aenv), 64, 64)}};
        ca.L[0] = chain_layer(E, in, 0, wt(p->blob.latent[l].wtq[1]), S, 64, cn, nullptr, &zz, &ad, 0, 0, 0);
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.latent[l].wtq[0]), 64, S * (l + 1) + u, c1, acc1, nullptr, nullptr, 1, -1, 0);
        return run_chain(ca, "B2");
      }
      case LatentReverse::FoldedChain:
      case LatentReverse::Resident:
        // the readout-reverse chain already applied Wout_0^T (folded into its lat0 columns): what is left of the output layer's
        // reverse is elementwise -- d h = (d a_0 + d a_0 of the moments) x silu'(h) -- and rides as the operand transform of the
        // first-layer reverse: ONE layer, 4 steps instead of 6
        ca.nlayers = 1;
        ca.L[0] = chain_layer(E, in, 0, wt(p->blob.latent[l].wtq[0]), 64, S * (l + 1) + u, c1, acc1, nullptr, nullptr, 0, -1, 0);
        ca.L[0].a_mode = 2;
        ca.L[0].a2_add = buf(w.g_aenv);
        ca.L[0].ld_a2add = 64;
        ca.L[0].a2_z = buf(w.lat_h[l][0]);
        ca.L[0].ld_a2z = 64;
        if (sp.latent_reverse == LatentReverse::FoldedChain) return run_chain(ca, "B2");
        {
          // the same layer with its 48 KB of weights resident in LDS (aa_chain_res.hip): one persistent workgroup per CU, no
          // per-workgroup staging, no barriers in the row loop
          ChainB2Args b2{};
          b2.M = E;
          b2.a = reinterpret_cast<const float*>(buf(w.g_fcat)) + S * (l + 1);
          b2.lda = SL1;
          b2.add = reinterpret_cast<const float*>(buf(w.g_aenv));
          b2.ldadd = 64;
          b2.z = reinterpret_cast<const float*>(buf(w.lat_h[l][0]));
          b2.ldz = 64;
          b2.Wq = wt(p->blob.latent[l].wtq[0]);
          b2.c0 = reinterpret_cast<float*>(buf(w.g_fcat));
          b2.ldc0 = SL1;
          b2.c1 = reinterpret_cast<float*>(buf(w.g_scal[l]));
          b2.ldc1 = u;
          if (int rc = launch_chain_b2_resident(b2, stream)) return rc;
          return mark("gc_64x128", gemm_row_elems(ca.L[0].g, true) + 2.0 * 64, 0, 2.0 * double(E) * 64 * 128);
        }
    }
    return fail(AA_ERR_INVALID, "step plan: unknown latent reverse form");
  }

  // reverse of tensor-product layer l
  int bwd_tp_layer(const aa_graph* g, int l) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, u = c.num_tensor, L = c.num_layers, W = p->W;
    switch (p->pipe.tp) {
      case TpPath::Operator:
        return run_op_bwd(g, l);
      case TpPath::Moments: {
        // (ran in the deep tail of the fused forward: the layer-1 slab of d Y is in the workspace, d a_0 was consumed there)
        if (l == 1 && sp.reverse_in_forward == ReverseInForward::ChainMomentsLatent0) return AA_OK;
        TpMomArgs m = mom_args(g);
        m.c.gscal0 = buf(w.g_scal[0]);
        m.c.gscal1 = buf(w.g_scal[1]);
        m.c.g_w0 = buf(w.g_w0);
        m.c.gsh_x1 = buf(w.g_sh);
        m.c.gsh_env = buf(w.g_sh) + size_t(l + 1) * size_t(E) * p->D;
        m.g_a = buf(w.g_aenv);
        if (l == 1) {
          m.ld_ga = c.latent_mlp_width;
          if (int rc = launch_tp_mom_bwd_last<T>(p->pipe.chain_pair, m, stream)) return rc;
          return mark("tp_mom_bwd_last", p->D + W + u + 2 * m.ka1 + p->D, double(p->D) * u);
        }
        m.ld_ga = S;
        // (after a fused forward the embedding's slot holds a_e = silu(h) of scalar_embed_mlp and the env weights are folded behind
        //  its output layer, fold_embed_output: d a_e comes out instead of d emb)
        if (sp.folded_first_stage()) m.wt0 = wt(p->blob.o_wt0f);
        if (sp.mom0_in_chain) {
          // stops after GM0 (in the slot of d a_e, which this form never writes): no read of a_e, no d a_e, no layer-0 slab of d Y here
          m.gm0 = buf(w.g_aenv);
          if (int rc = launch_tp_mom_bwd_first_gm(p->pipe.chain_pair, m, stream)) return rc;
          return mark("tp_mom_bwd_first", p->D + 2 * W + 2 * u + p->D, double(p->D) * 64, 2.0 * p->D * u);
        }
        if (int rc = launch_tp_mom_bwd_first<T>(p->pipe.chain_pair, m, stream)) return rc;
        return mark("tp_mom_bwd_first", p->D + 2 * W + 2 * u + 2 * m.ka0 + 2 * p->D, 2.0 * p->D * u);
      }
      case TpPath::SpecChain: {
        TpChainArgs a = chain_args(g);
        a.gscal0 = buf(w.g_scal[0]);
        a.gscal1 = buf(w.g_scal[1]);
        a.g_w0 = buf(w.g_w0);
        a.g_wenv = buf(w.g_envw);
        a.gsh_x1 = buf(w.g_sh);
        a.gsh_env = buf(w.g_sh) + size_t(l + 1) * size_t(E) * p->D;
        if (l == 1) {
          if (int rc = launch_tp_chain_bwd_last<T>(p->pipe.chain_pair, a, stream)) return rc;
          return mark("tp_chain_bwd_last", 3 * W + 2 * p->D + u, 2.0 * p->D * u);
        }
        if (int rc = launch_tp_chain_bwd_first<T>(p->pipe.chain_pair, a, stream)) return rc;
        return mark("tp_chain_bwd_first", 4 * W + 3 * p->D + 2 * u, 2.0 * p->D * u);
      }
      case TpPath::Spec: {
        TpSpecBwdArgs a{};
        spec_operands(a, g, l);
        if (l == 0) {
          a.g_w1 = buf(w.g_w0);
          a.ld_gw1 = W;
        } else {
          a.g_x1_dense = buf(w.g_tf[(l - 1) & 1]);
        }
        a.gout = l < L - 1 ? buf(w.g_tf[l & 1]) : nullptr;
        a.gscal = buf(w.g_scal[l]);
        a.ld_gscal = u;
        a.g_wenv = buf(w.g_envw);
        a.ld_gwe = W;
        a.gsh_x1 = buf(w.g_sh);
        a.gsh_env = buf(w.g_sh) + size_t(l + 1) * size_t(E) * p->D;
        a.ld_gsh = p->D;
        if (int rc = launch_tp_spec_bwd<T>(p->pipe.spec_sig[l], a, stream)) return rc;
        return mark("tp_spec_bwd", 4 * W + 3 * p->D + 2 * u * p->D + u, 2.0 * p->D * u);
      }
      case TpPath::General: {
        TpLayerBwdArgs a{};
        general_operands(a, g, l);
        a.gout = l < L - 1 ? buf(w.g_tf[l & 1]) : nullptr;
        a.gscal = buf(w.g_scal[l]);
        a.ld_gscal = u;
        if (l == 0) {
          a.g1.gw = buf(w.g_w0);
          a.g1.ldgw = W;
          a.g1.gsh = buf(w.g_sh);
          a.g1.ld_gsh = p->D;
        } else {
          a.g1.dense = buf(w.g_tf[(l - 1) & 1]);
        }
        a.g2.gw = buf(w.g_envw);
        a.g2.ldgw = W;
        a.g2.gsh = buf(w.g_sh);
        a.g2.ld_gsh = p->D;
        if (int rc = launch_tp_layer_bwd<T>(p->layers[l], a, stream)) return rc;
        return mark("tp_layer_bwd", 4 * W + 2 * p->D + 2 * u * p->D + u, 2.0 * p->D * u);
      }
    }
    return fail(AA_ERR_INVALID, "step plan: unknown tensor-product path");
  }

  // first-stage reverse + scalar_embed_mlp reverse
  int bwd_first_stage(const aa_graph* g) {
    const aa_model_config& c = p->cfg;
    const int S = c.num_scalar, W = p->W, SL1 = p->SL1;
    if (!p->pipe.chains()) {
      // fused first stage reverse
      {
        SegList go{3, {seg(buf(w.g_fcat), SL1, S), seg(buf(w.g_w0), W, W), seg(buf(w.g_envw), W, W)}};
        if (p->pipe.env_moments()) go.count = 2;
        SegList gi{1, {seg(buf(w.g_emb), S, S)}};
        SegList aenv{1, {seg(p->pipe.env_moments() ? buf(w.g_aenv) : nullptr, S, S)}};
        act_now = AA_ACT_SILU;
        if (int rc = gemm(go, 0, wt(p->blob.o_g0t), wt(p->blob.o_g0tp), wt(p->blob.o_g0tq), p->blob.ng0, S, gi, nullptr, nullptr,
                          p->pipe.env_moments() ? &aenv : nullptr))
          return rc;
      }
      // scalar_embed_mlp reverse
      SegList go{1, {seg(buf(w.g_emb), S, S)}};
      SegList gi{1, {seg(buf(w.g_emb0), c.embed_dim, c.embed_dim)}};
      return mlp_bwd(p->blob.embed, c.embed_mlp_depth + 1, go, w.se_h, w.g_se_h, gi, nullptr, 0);
    }
    // ... in ONE kernel
    const SegList none{0, {}};
    ChainArgs ca{};
    ca.nlayers = 3;
    SegList in{2, {seg(buf(w.g_fcat), SL1, S), seg(buf(w.g_w0), W, W)}};
    SegList cn{1, {seg(nullptr, 64, 64)}};
    SegList ad{1, {seg(buf(w.g_aenv), S, S)}};
    SegList zz{1, {seg(buf(w.se_h[0]), 64, 64)}};
    SegList ce{1, {seg(buf(w.g_emb0), c.embed_dim, c.embed_dim)}};
    ca.L[0] = chain_layer(E, in, 0, wt(p->blob.o_g0tq), p->blob.ng0, S, cn, nullptr, nullptr, &ad, 0, 0, 0);
    ca.L[1] = chain_layer(E, none, 0, wt(p->blob.embed.wtq[1]), S, 64, cn, nullptr, &zz, nullptr, 1, 0, 0);
    ca.L[2] = chain_layer(E, none, 0, wt(p->blob.embed.wtq[0]), 64, c.embed_dim, ce, nullptr, nullptr, nullptr, 1, -1, 0);
    // the epilogue that contracts d (two-body embedding) straight back to the 8 basis functions (ModelPipeline::embed_fused)
    auto contract_embedding = [&](ChainLayer& layer, const T* table) {
      layer.embrev_out = buf(w.trev);
      ca.emb_table = table;
      ca.num_types = c.num_types;
      ca.types = g->types;
      ca.center = g->center;
      ca.nbr = g->nbr;
    };
    if (sp.folded_first_stage()) {
      // everything in front of the hidden layer of scalar_embed_mlp folded (fold_embed_output; the forward stored a_e, not the embedding):
      // d h = ((d[two-body | w0] @ (W1 G0)^T) + d a_e of the moments) x silu'(h) -- ONE 256 -> 64 layer, 8 steps -- ...
      ca.nlayers = 1;
      ca.L[0] = chain_layer(E, in, 0, wt(p->blob.o_g0tfq), p->blob.ng0, 64, cn, nullptr, &zz, &ad, 0, 0, 0);
      if (sp.mom0_in_chain) {
        // ... with d a_e of the moments formed in the epilogue from GM0 of the row's center atom (tp_mom_bwd_first stopped there), which
        // also writes the layer-0 slab of d Y: the silu'(h) factor and the addend are the epilogue's own
        ca.L[0] = chain_layer(E, in, 0, wt(p->blob.o_g0tfq), p->blob.ng0, 64, cn, nullptr, nullptr, nullptr, 0, 0, 0);
        ca.L[0].mom_gm0 = buf(w.g_aenv);
        ca.L[0].mom_d = p->D;
        ca.L[0].mom_y = buf(w.sh);
        ca.L[0].ld_mom_y = p->D;
        ca.L[0].mom_h = buf(w.se_h[0]);
        ca.L[0].ld_mom_h = 64;
        ca.L[0].mom_dy = buf(w.g_sh) + size_t(E) * p->D;
        ca.L[0].ld_mom_dy = p->D;
      }
      if (p->pipe.embed_fused && p->pipe.fold_embed_table) {
        // ... contracted against the folded two-body table in its epilogue
        contract_embedding(ca.L[0], wt(p->blob.o_embtab_h));
      } else {
        // ... (three species: no table in the chain's LDS) followed by W0^T -> d emb0 for the edge reverse
        ca.nlayers = 2;
        ca.L[1] = chain_layer(E, none, 0, wt(p->blob.embed.wtq[0]), 64, c.embed_dim, ce, nullptr, nullptr, nullptr, 1, -1, 0);
      }
    } else if (p->pipe.embed_fused && p->pipe.fold_embed_table) {
      // folded table (fold_embed_table): d_h, the output of the second layer, is contracted straight back to the 8 basis functions
      // with T = tab @ W0 -- the layer W0^T and d emb0 do not exist
      ca.nlayers = 2;
      contract_embedding(ca.L[1], wt(p->blob.o_embtab_h));
    } else if (p->pipe.embed_fused) {
      // d emb0 is contracted straight back to the 8 basis functions in the epilogue and never stored
      ca.L[2].g.c = SegList{1, {seg(nullptr, c.embed_dim, c.embed_dim)}};
      contract_embedding(ca.L[2], wt(p->blob.o_embtab));
    }
    return run_chain(ca, "B1");
  }

  // The reverse pass w.r.t. positions, top down; the stages the forward of this step already ran (StepPlan::reverse_in_forward)
  // launch nothing.
  int backward(const aa_graph* g, const void* pos, void* forces) {
    if (sp.slot) return backward_slot(g, pos, forces);
    if (int rc = bwd_begin(forces)) return rc;
    if (int rc = bwd_readout(g)) return rc;
    for (int l = p->cfg.num_layers - 1; l >= 0; --l) {
      if (int rc = bwd_latent(l)) return rc;
      if (int rc = bwd_tp_layer(g, l)) return rc;
    }
    if (int rc = bwd_first_stage(g)) return rc;
    return edge_tail(g, pos, forces);
  }
};

// what makes a step one block of a blocked step: rows of the frame-wide vec / dvec arrays at the block's first edge (force steps; both
// null on an energy-only one)
struct BlockStep {
  void* vec = nullptr;
  void* dvec = nullptr;
};

template <typename T>
int run_model(const aa_model_plan* p, const void* dev_weights, const aa_graph* g, const void* pos, void* workspace,
              size_t ws_bytes, void* atom_energy, void* forces, hipStream_t stream, StageProfile* prof = nullptr,
              const BlockStep* blk = nullptr) {
  Runner<T> r;
  r.prof = prof;
  if (blk) {
    r.frame_vec = blk->vec;
    r.frame_dvec = blk->dvec;
  }
  r.p = p;
  r.wts = static_cast<const T*>(dev_weights);
  r.ws = static_cast<char*>(workspace);
  r.E = g->num_edges;
  r.N = g->num_atoms;
  r.stream = stream;
  r.e_out = atom_energy;
  r.w = layout_workspace(p, r.N, r.E, forces != nullptr);
  if (r.w.total > ws_bytes) return fail(AA_ERR_WORKSPACE, "aa_model_energy_forces: workspace too small");
  if (p->opt.poison_workspace) AA_CHECK_HIP(hipMemsetAsync(workspace, 0xFF, r.w.total, stream));  // debugging: NaN everywhere
  StepInputs in{};
  in.f32 = sizeof(T) == 4;
  in.taps = p->taps;
  in.with_forces = forces != nullptr;
  in.transposed_csr = g->t_rowptr && g->t_perm;
  in.atoms = g->num_atoms;
  in.edges = g->num_edges;
  in.atom0 = r.atom_begin(g);
  in.atom_end = r.atom_end(g);
  in.max_degree = g->max_degree;
  in.pair_zbl = p->zbl_tab != nullptr;
  in.block = blk != nullptr;
  int cus = 0;  // (asked only where a decision reads it)
  if (wide_one_tile_pass(p->pipe, choose_forward(p->pipe, p->opt, p->cfg, in)) && (cus = device_cu_count()) < 0) return cus;
  r.sp = choose_step(p->pipe, p->opt, p->cfg, in, cus);
  if (p->ev_wait && !blk) AA_CHECK_HIP(hipStreamWaitEvent(stream, (hipEvent_t)(uintptr_t)(p->ev_wait), 0));
  if (int rc = r.forward(g, pos, atom_energy)) return rc;
  if (p->ev_record && !blk) AA_CHECK_HIP(hipEventRecord((hipEvent_t)(uintptr_t)(p->ev_record), stream));
  if (forces) {
    if (int rc = r.backward(g, pos, forces)) return rc;  // (ends in edge_tail, which launches the pair potential of a force step)
  } else if (r.sp.pair_zbl) {
    if (int rc = r.pair_zbl(g, pos, nullptr)) return rc;
  }
  // the atom-block hint is the caller's promise (per-atom kernels skip the rest): two row pointers verify it on the device, as the
  // LAST launch of the step, so that a broken promise also turns this step's energies and forces into NaN
  // (a block of a blocked step: its row pointers are clamped to the block, launch_block_rowptr has checked the cut)
  if (!blk && g->atom_end > g->atom_begin && (g->atom_begin > 0 || g->atom_end < g->num_atoms) && p->status)
    if (int rc = launch_graph_hint_check(g->rowptr, g->num_atoms, g->atom_begin, g->atom_end, p->status, atom_energy, forces, int(sizeof(T)), stream))
      return rc;
  return AA_OK;
}
}  // namespace

extern "C" int aa_model_energy_forces(const aa_model_plan* plan, const void* dev_weights, const aa_graph* graph,
                                      const void* pos, void* workspace, size_t workspace_bytes, void* atom_energy,
                                      void* forces, aa_stream stream) {
  AA_REQUIRE(plan && dev_weights && graph && pos && atom_energy, "aa_model_energy_forces: null argument");
  AA_REQUIRE(graph->num_atoms >= 0 && graph->num_edges >= 0 && graph->num_edges < (int64_t(1) << 31),
             "aa_model_energy_forces: graph too large for int32 edge ids");
  AA_REQUIRE(graph->num_edges == 0 || (graph->center && graph->nbr), "aa_model_energy_forces: null edge arrays");
  AA_REQUIRE(graph->rowptr && graph->types, "aa_model_energy_forces: null rowptr/types");
  AA_REQUIRE(graph->atom_begin >= 0 && graph->atom_end <= graph->num_atoms &&
                 (graph->atom_end >= graph->atom_begin || graph->atom_end == 0),
             "aa_model_energy_forces: atom_begin/atom_end out of range");
  AA_REQUIRE(workspace || workspace_bytes == 0, "aa_model_energy_forces: null workspace");
  if (int rc = consume_status(plan, "aa_model_energy_forces")) return rc;  // (an EARLIER step contradicted the graph hints)
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto run = [&](hipStream_t st) {
    if (plan->cfg.dtype == AA_F32)
      return run_model<float>(plan, dev_weights, graph, pos, workspace, workspace_bytes, atom_energy, forces, st);
    return run_model<double>(plan, dev_weights, graph, pos, workspace, workspace_bytes, atom_energy, forces, st);
  };
  aa_model_plan::StepGraph& sg = plan->sg;
  if (!sg.enabled) return run(s);
  const aa_model_plan::StepGraph::Key key{dev_weights,    pos,           workspace,     atom_energy,      forces,          graph->center,
                                          graph->nbr,     graph->rowptr, graph->types,  graph->shift_vec, graph->t_rowptr, graph->t_perm,
                                          graph->num_atoms, graph->num_edges, graph->atom_begin, graph->atom_end,
                                          workspace_bytes, graph->max_degree, plan->taps ? 1 : 0};
  if (!sg.exec || !(sg.key == key)) {
    if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
    if (sg.graph) (void)hipGraphDestroy(sg.graph);
    sg.exec = nullptr;
    sg.graph = nullptr;
    AA_CHECK_HIP(hipStreamBeginCapture(sg.cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = run(sg.cap_stream);
    const hipError_t ec = hipStreamEndCapture(sg.cap_stream, &sg.graph);
    if (rc != AA_OK) return rc;
    if (ec != hipSuccess) return fail(AA_ERR_HIP, "aa_model_energy_forces: graph capture failed");
    AA_CHECK_HIP(hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0));
    sg.key = key;
  }
  AA_CHECK_HIP(hipGraphLaunch(sg.exec, s));
  return AA_OK;
}

extern "C" int aa_model_energy_forces_profiled(const aa_model_plan* plan, const void* dev_weights, const aa_graph* graph,
                                               const void* pos, void* workspace, size_t workspace_bytes,
                                               void* atom_energy, void* forces, aa_stream stream, int max_stages,
                                               float* stage_ms, char* stage_names /* [max_stages][32] */,
                                               int* num_stages, double* stage_bytes, double* stage_flops) {
  AA_REQUIRE(plan && dev_weights && graph && pos && atom_energy && stage_ms && stage_names && num_stages,
             "aa_model_energy_forces_profiled: null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  StageProfile prof;
  int rc = plan->cfg.dtype == AA_F32
               ? run_model<float>(plan, dev_weights, graph, pos, workspace, workspace_bytes, atom_energy, forces, s, &prof)
               : run_model<double>(plan, dev_weights, graph, pos, workspace, workspace_bytes, atom_energy, forces, s, &prof);
  if (rc == AA_OK) {
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(AA_ERR_HIP, "profile: stream sync failed");
  }
  int n = 0;
  if (rc == AA_OK) {
    for (size_t i = 1; i < prof.events.size() && n < max_stages; ++i, ++n) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, prof.events[i - 1], prof.events[i]);
      stage_ms[n] = ms;
      snprintf(stage_names + 32 * n, 32, "%s", prof.names[i].c_str());
      if (stage_bytes) stage_bytes[n] = prof.bytes[i];
      if (stage_flops) stage_flops[n] = prof.flops[i];
    }
  }
  *num_stages = n;
  prof.clear();
  return rc;
}

// ------------------------------------------------------------------------------------------------
// blocked step: the frame one block of center atoms after the other, in one arena
// ------------------------------------------------------------------------------------------------
namespace {
template <typename T>
int run_blocked(const aa_model_plan* p, const void* dev_weights, const aa_graph* g, const void* pos, int32_t num_blocks, const int64_t* block_atoms,
                const int64_t* block_edges, const BlockedWorkspace& bw, char* base, void* atom_energy, void* forces, hipStream_t stream) {
  const int64_t N = g->num_atoms;
  int32_t* rowptr_b = reinterpret_cast<int32_t*>(base + bw.rowptr);
  int32_t* bad = reinterpret_cast<int32_t*>(base + bw.bad);
  if (p->opt.poison_workspace) AA_CHECK_HIP(hipMemsetAsync(base, 0xFF, bw.total, stream));  // (the frame part too; every block poisons the arena again)
  AA_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), stream));
  for (int32_t b = 0; b < num_blocks; ++b) {
    const int64_t a0 = block_atoms[b], a1 = block_atoms[b + 1], lo = block_edges[b], hi = block_edges[b + 1];
    if (a1 == a0 && hi == lo) continue;  // nothing to evaluate (its two cuts are those of its neighbours, which check them)
    if (int rc = launch_block_rowptr(g->rowptr, N, a0, a1, int32_t(lo), int32_t(hi), b, rowptr_b, p->status, bad, stream)) return rc;
    if (a1 == a0) continue;  // (edges without an atom: a wrong cut, just reported)
    aa_graph sub = *g;
    sub.num_edges = hi - lo;
    sub.center = g->center ? g->center + lo : nullptr;
    sub.nbr = g->nbr ? g->nbr + lo : nullptr;
    sub.rowptr = rowptr_b;
    sub.shift_vec = g->shift_vec ? static_cast<const char*>(g->shift_vec) + size_t(lo) * 3 * sizeof(T) : nullptr;
    sub.t_rowptr = nullptr;  // (no block assembles forces)
    sub.t_perm = nullptr;
    sub.atom_begin = a0;
    sub.atom_end = a1;
    BlockStep blk{};
    if (forces) {
      blk.vec = base + bw.vec + size_t(lo) * 4 * sizeof(T);
      blk.dvec = base + bw.dvec + size_t(lo) * 4 * sizeof(T);
    }
    if (int rc = run_model<T>(p, dev_weights, &sub, pos, base, bw.arena.total, atom_energy, forces, stream, nullptr, &blk)) return rc;
  }
  if (forces) {
    // ONE deterministic force assembly over the frame arrays: the summation order of the unblocked step with a transposed CSR
    ForceGatherArgs fg{N, g->rowptr, g->t_rowptr, g->t_perm, base + bw.dvec, forces};
    if (int rc = launch_force_gather<T>(fg, stream)) return rc;
  }
  return launch_blocked_finish(bad, N, atom_energy, forces, int(sizeof(T)), stream);
}
}  // namespace

extern "C" int aa_model_energy_forces_blocked(const aa_model_plan* plan, const void* dev_weights, const aa_graph* graph, const void* pos,
                                              int32_t num_blocks, const int64_t* block_atoms, const int64_t* block_edges, void* workspace,
                                              size_t workspace_bytes, void* atom_energy, void* forces, aa_stream stream) {
  const char* who = "aa_model_energy_forces_blocked";
  AA_REQUIRE(plan && dev_weights && graph && pos && atom_energy && block_atoms && block_edges, "aa_model_energy_forces_blocked: null argument");
  AA_REQUIRE(graph->num_atoms >= 0 && graph->num_edges >= 0 && graph->num_edges < (int64_t(1) << 31),
             "aa_model_energy_forces_blocked: graph too large for int32 edge ids");
  AA_REQUIRE(graph->num_edges == 0 || (graph->center && graph->nbr), "aa_model_energy_forces_blocked: null edge arrays");
  AA_REQUIRE(graph->rowptr && graph->types, "aa_model_energy_forces_blocked: null rowptr/types");
  AA_REQUIRE(workspace, "aa_model_energy_forces_blocked: null workspace");
  AA_REQUIRE(num_blocks >= 1, "aa_model_energy_forces_blocked: num_blocks must be at least 1");
  if (plan->sg.enabled)
    return fail(AA_ERR_INVALID, std::string(who) + ": the blocked step is not captured into a hipGraph (aa_model_plan_enable_graph is on for this plan; "
                                                   "its launch list depends on the block cuts)");
  if (plan->taps)
    return fail(AA_ERR_INVALID, std::string(who) + ": the blocked step does not serve the debug taps (aa_model_plan_enable_taps is on for this plan; "
                                                   "the arena holds one block at a time)");
  if (forces && !(graph->t_rowptr && (graph->t_perm || graph->num_edges == 0)))
    return fail(AA_ERR_INVALID, std::string(who) + ": forces are assembled once over the whole frame through the transposed CSR "
                                                   "(aa_graph.t_rowptr / t_perm, aa_graph_transpose); there is no atomics fallback");
  const int64_t N = graph->num_atoms, E = graph->num_edges;
  if (block_atoms[0] != 0 || block_atoms[num_blocks] != N)
    return fail(AA_ERR_INVALID, std::string(who) + ": block_atoms must run from 0 to num_atoms (block_atoms[0] = " + std::to_string(block_atoms[0]) +
                                    ", block_atoms[" + std::to_string(num_blocks) + "] = " + std::to_string(block_atoms[num_blocks]) + ", num_atoms = " +
                                    std::to_string(N) + ")");
  if (block_edges[0] != 0 || block_edges[num_blocks] != E)
    return fail(AA_ERR_INVALID, std::string(who) + ": block_edges must run from 0 to num_edges (block_edges[0] = " + std::to_string(block_edges[0]) +
                                    ", block_edges[" + std::to_string(num_blocks) + "] = " + std::to_string(block_edges[num_blocks]) + ", num_edges = " +
                                    std::to_string(E) + ")");
  int64_t cap = 0;
  for (int32_t b = 0; b < num_blocks; ++b) {
    if (block_atoms[b + 1] < block_atoms[b])
      return fail(AA_ERR_INVALID, std::string(who) + ": block_atoms must be non-decreasing (block " + std::to_string(b) + ")");
    if (block_edges[b + 1] < block_edges[b])
      return fail(AA_ERR_INVALID, std::string(who) + ": block_edges must be non-decreasing (block " + std::to_string(b) + ")");
    cap = std::max(cap, block_edges[b + 1] - block_edges[b]);
  }
  if (int rc = consume_status(plan, who)) return rc;  // (an EARLIER step contradicted its graph hints or its cuts)
  const BlockedWorkspace bw = layout_blocked(plan, N, E, cap, forces != nullptr);
  if (bw.total > workspace_bytes)
    return fail(AA_ERR_WORKSPACE, std::string(who) + ": workspace too small (aa_model_blocked_workspace_bytes at the largest block, " + std::to_string(cap) +
                                      " edges, asks for " + std::to_string(bw.total) + " bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  return plan->cfg.dtype == AA_F32
             ? run_blocked<float>(plan, dev_weights, graph, pos, num_blocks, block_atoms, block_edges, bw, base, atom_energy, forces, s)
             : run_blocked<double>(plan, dev_weights, graph, pos, num_blocks, block_atoms, block_edges, bw, base, atom_energy, forces, s);
}

// ------------------------------------------------------------------------------------------------
// What is read off a finished force step: the virial, the per-atom virial and the potential part of the heat flux, each from the
// [E,4] rows the step left in its workspace.  Where those rows lie -- the unblocked step's workspace or the blocked step's frame
// arrays -- is all that differs between an entry point and its blocked twin, and locate_step_rows answers it.
// ------------------------------------------------------------------------------------------------
namespace {
// where a force step left its [E,4] rows and the reduction scratch
struct StepRows {
  char *vec, *dvec, *vir_part;
};

// The rows of the step that ran in `workspace`: the unblocked one (max_block_edges < 0) or the blocked one at this max_block_edges.
// Refuses, in the name of `who`, a workspace smaller than that step's.
int locate_step_rows(const aa_model_plan* plan, const aa_graph* graph, int64_t max_block_edges, void* workspace, size_t workspace_bytes,
                     const char* who, StepRows* out) {
  char* base = static_cast<char*>(workspace);
  if (max_block_edges < 0) {
    const Workspace w = layout_workspace(plan, graph->num_atoms, graph->num_edges, 1);
    if (w.total > workspace_bytes) return fail(AA_ERR_WORKSPACE, std::string(who) + ": workspace too small (was it sized with forces?)");
    *out = StepRows{base + w.vec, base + w.dvec, base + w.vir_part};
    return AA_OK;
  }
  const BlockedWorkspace bw = layout_blocked(plan, graph->num_atoms, graph->num_edges, std::min(max_block_edges, graph->num_edges), 1);
  if (bw.total > workspace_bytes)
    return fail(AA_ERR_WORKSPACE, std::string(who) + ": workspace too small (was it sized with forces, at this max_block_edges?)");
  *out = StepRows{base + bw.vec, base + bw.dvec, base + bw.arena.vir_part};
  return AA_OK;
}

// Each body serves an entry point and its blocked twin: `who` names the caller in every message, max_block_edges < 0 is the unblocked step.

int virial_from(const aa_model_plan* plan, const aa_graph* graph, const char* who, int64_t max_block_edges, void* workspace,
                size_t workspace_bytes, void* virial9, aa_stream stream) {
  StepRows r;
  if (int rc = locate_step_rows(plan, graph, max_block_edges, workspace, workspace_bytes, who, &r)) return rc;
  VirialArgs a{graph->num_edges, r.dvec, r.vec, reinterpret_cast<double*>(r.vir_part), virial9};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return plan->cfg.dtype == AA_F32 ? launch_virial<float>(a, s) : launch_virial<double>(a, s);
}

int atom_virial_from(const aa_model_plan* plan, const aa_graph* graph, const char* who, int64_t max_block_edges, void* workspace,
                     size_t workspace_bytes, int attribution, void* out_n9, aa_stream stream) {
  double cc, cn;
  switch (attribution) {
    case AA_ATOM_VIRIAL_CENTER: cc = 1.0, cn = 0.0; break;
    case AA_ATOM_VIRIAL_NEIGHBOR: cc = 0.0, cn = 1.0; break;
    case AA_ATOM_VIRIAL_SPLIT: cc = cn = 0.5; break;
    default: return fail(AA_ERR_INVALID, std::string(who) + ": unknown attribution " + std::to_string(attribution) +
                                             " (AA_ATOM_VIRIAL_CENTER, _NEIGHBOR or _SPLIT)");
  }
  // (no atomics fallback: a per-atom tensor that changes from call to call is what this entry point exists to avoid)
  // (a list without edges has row pointers and an EMPTY t_perm, which a host may well pass as a null pointer: nothing reads it)
  if (cn != 0.0 && !(graph->t_rowptr && (graph->t_perm || graph->num_edges == 0)))
    return fail(AA_ERR_INVALID, std::string(who) + ": the neighbor and split attributions need the transposed CSR "
                                                   "(aa_graph.t_rowptr / t_perm, aa_graph_transpose)");
  StepRows r;  // (located last: an unknown attribution or a missing transposed CSR is refused whatever the workspace)
  if (int rc = locate_step_rows(plan, graph, max_block_edges, workspace, workspace_bytes, who, &r)) return rc;
  AtomVirialArgs a{graph->num_atoms, graph->rowptr, graph->t_rowptr, graph->t_perm, r.dvec, r.vec, cc, cn, out_n9};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return plan->cfg.dtype == AA_F32 ? launch_atom_virial<float>(a, s) : launch_atom_virial<double>(a, s);
}

int heat_flux_from(const aa_model_plan* plan, const aa_graph* graph, const char* who, int64_t max_block_edges, void* workspace,
                   size_t workspace_bytes, const void* velocities, void* flux3, aa_stream stream) {
  StepRows r;
  if (int rc = locate_step_rows(plan, graph, max_block_edges, workspace, workspace_bytes, who, &r)) return rc;
  if (!flux3) return fail(AA_ERR_INVALID, std::string(who) + ": null flux3");
  if (!velocities && graph->num_atoms > 0) return fail(AA_ERR_INVALID, std::string(who) + ": null velocities");
  if (graph->num_edges > 0 && !graph->nbr) return fail(AA_ERR_INVALID, std::string(who) + ": null neighbor array (aa_graph.nbr)");
  HeatFluxArgs a{graph->num_edges, r.dvec, r.vec, graph->nbr, velocities, reinterpret_cast<double*>(r.vir_part), flux3};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return plan->cfg.dtype == AA_F32 ? launch_heat_flux<float>(a, s) : launch_heat_flux<double>(a, s);
}

// The per-frame sums of a batch (aa_frames): what the host can check of the descriptor, then one launch.  The edge sums find their
// rows as the bodies above do; their scratch is not used.
int check_frames(const aa_frames* frames, const char* who) {
  AA_REQUIRE(frames, std::string(who) + ": null frames");
  AA_REQUIRE(frames->num_frames >= 0, std::string(who) + ": negative num_frames");
  AA_REQUIRE(frames->frame_atoms || frames->num_frames == 0, std::string(who) + ": null frame_atoms");
  return AA_OK;
}

int frame_sum(const aa_model_plan* plan, FrameSumKind kind, const FrameSumArgs& a, aa_stream stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  return plan->cfg.dtype == AA_F32 ? launch_frame_sum<float>(kind, a, s) : launch_frame_sum<double>(kind, a, s);
}

int frame_edge_sum_from(const aa_model_plan* plan, const aa_graph* graph, const aa_frames* frames, FrameSumKind kind, const char* who,
                        int64_t max_block_edges, void* workspace, size_t workspace_bytes, const void* velocities, void* out, aa_stream stream) {
  if (int rc = check_frames(frames, who)) return rc;
  StepRows r;
  if (int rc = locate_step_rows(plan, graph, max_block_edges, workspace, workspace_bytes, who, &r)) return rc;
  if (!out && frames->num_frames > 0) return fail(AA_ERR_INVALID, std::string(who) + ": null output");
  if (!graph->rowptr) return fail(AA_ERR_INVALID, std::string(who) + ": null row pointers (aa_graph.rowptr)");
  if (kind == FRAME_FLUX) {
    if (!velocities && graph->num_atoms > 0) return fail(AA_ERR_INVALID, std::string(who) + ": null velocities");
    if (graph->num_edges > 0 && !graph->nbr) return fail(AA_ERR_INVALID, std::string(who) + ": null neighbor array (aa_graph.nbr)");
  }
  FrameSumArgs a{frames->num_frames, frames->frame_atoms, graph->num_atoms, graph->num_edges, graph->rowptr, r.dvec, r.vec, graph->nbr,
                 velocities, plan->status, out};
  return frame_sum(plan, kind, a, stream);
}
}  // namespace

// The entry points: null checks, the blocked ones refuse a negative max_block_edges, then the body.

extern "C" int aa_model_virial(const aa_model_plan* plan, const aa_graph* graph, void* workspace, size_t workspace_bytes,
                               void* virial9, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace && virial9, "aa_model_virial: null argument");
  return virial_from(plan, graph, "aa_model_virial", -1, workspace, workspace_bytes, virial9, stream);
}

extern "C" int aa_model_blocked_virial(const aa_model_plan* plan, const aa_graph* graph, int64_t max_block_edges, void* workspace,
                                       size_t workspace_bytes, void* virial9, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace && virial9, "aa_model_blocked_virial: null argument");
  AA_REQUIRE(max_block_edges >= 0, "aa_model_blocked_virial: negative max_block_edges");
  return virial_from(plan, graph, "aa_model_blocked_virial", max_block_edges, workspace, workspace_bytes, virial9, stream);
}

extern "C" int aa_model_atom_virial(const aa_model_plan* plan, const aa_graph* graph, void* workspace, size_t workspace_bytes,
                                    int attribution, void* out_n9, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace && out_n9, "aa_model_atom_virial: null argument");
  return atom_virial_from(plan, graph, "aa_model_atom_virial", -1, workspace, workspace_bytes, attribution, out_n9, stream);
}

extern "C" int aa_model_blocked_atom_virial(const aa_model_plan* plan, const aa_graph* graph, int64_t max_block_edges, void* workspace,
                                            size_t workspace_bytes, int attribution, void* out_n9, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace && out_n9, "aa_model_blocked_atom_virial: null argument");
  AA_REQUIRE(max_block_edges >= 0, "aa_model_blocked_atom_virial: negative max_block_edges");
  return atom_virial_from(plan, graph, "aa_model_blocked_atom_virial", max_block_edges, workspace, workspace_bytes, attribution, out_n9, stream);
}

extern "C" int aa_model_heat_flux(const aa_model_plan* plan, const aa_graph* graph, void* workspace, size_t workspace_bytes,
                                  const void* velocities, void* flux3, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace, "aa_model_heat_flux: null argument");
  return heat_flux_from(plan, graph, "aa_model_heat_flux", -1, workspace, workspace_bytes, velocities, flux3, stream);
}

extern "C" int aa_model_blocked_heat_flux(const aa_model_plan* plan, const aa_graph* graph, int64_t max_block_edges, void* workspace,
                                          size_t workspace_bytes, const void* velocities, void* flux3, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace, "aa_model_blocked_heat_flux: null argument");
  AA_REQUIRE(max_block_edges >= 0, "aa_model_blocked_heat_flux: negative max_block_edges");
  return heat_flux_from(plan, graph, "aa_model_blocked_heat_flux", max_block_edges, workspace, workspace_bytes, velocities, flux3, stream);
}

extern "C" int aa_model_frame_energies(const aa_model_plan* plan, const aa_frames* frames, int64_t num_atoms, const void* atom_energy,
                                       void* out_b, aa_stream stream) {
  const char* who = "aa_model_frame_energies";
  AA_REQUIRE(plan, "aa_model_frame_energies: null plan");
  if (int rc = check_frames(frames, who)) return rc;
  AA_REQUIRE(num_atoms >= 0, "aa_model_frame_energies: negative num_atoms");
  AA_REQUIRE(atom_energy || num_atoms == 0, "aa_model_frame_energies: null atom_energy");
  AA_REQUIRE(out_b || frames->num_frames == 0, "aa_model_frame_energies: null output");
  FrameSumArgs a{frames->num_frames, frames->frame_atoms, num_atoms, 0, nullptr, atom_energy, nullptr, nullptr, nullptr, plan->status, out_b};
  return frame_sum(plan, FRAME_ENERGY, a, stream);
}

extern "C" int aa_model_frame_virial(const aa_model_plan* plan, const aa_graph* graph, const aa_frames* frames, void* workspace,
                                     size_t workspace_bytes, void* out_b9, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace, "aa_model_frame_virial: null argument");
  return frame_edge_sum_from(plan, graph, frames, FRAME_VIRIAL, "aa_model_frame_virial", -1, workspace, workspace_bytes, nullptr, out_b9, stream);
}

extern "C" int aa_model_blocked_frame_virial(const aa_model_plan* plan, const aa_graph* graph, int64_t max_block_edges, const aa_frames* frames,
                                             void* workspace, size_t workspace_bytes, void* out_b9, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace, "aa_model_blocked_frame_virial: null argument");
  AA_REQUIRE(max_block_edges >= 0, "aa_model_blocked_frame_virial: negative max_block_edges");
  return frame_edge_sum_from(plan, graph, frames, FRAME_VIRIAL, "aa_model_blocked_frame_virial", max_block_edges, workspace, workspace_bytes,
                             nullptr, out_b9, stream);
}

extern "C" int aa_model_frame_heat_flux(const aa_model_plan* plan, const aa_graph* graph, const aa_frames* frames, void* workspace,
                                        size_t workspace_bytes, const void* velocities, void* out_b3, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace, "aa_model_frame_heat_flux: null argument");
  return frame_edge_sum_from(plan, graph, frames, FRAME_FLUX, "aa_model_frame_heat_flux", -1, workspace, workspace_bytes, velocities, out_b3, stream);
}

extern "C" int aa_model_blocked_frame_heat_flux(const aa_model_plan* plan, const aa_graph* graph, int64_t max_block_edges,
                                                const aa_frames* frames, void* workspace, size_t workspace_bytes, const void* velocities,
                                                void* out_b3, aa_stream stream) {
  AA_REQUIRE(plan && graph && workspace, "aa_model_blocked_frame_heat_flux: null argument");
  AA_REQUIRE(max_block_edges >= 0, "aa_model_blocked_frame_heat_flux: negative max_block_edges");
  return frame_edge_sum_from(plan, graph, frames, FRAME_FLUX, "aa_model_blocked_frame_heat_flux", max_block_edges, workspace, workspace_bytes,
                             velocities, out_b3, stream);
}

extern "C" int aa_model_debug_tap(const aa_model_plan* plan, const char* name, int64_t N, int64_t E, const void* workspace,
                                  const void** ptr, int64_t* ld) {
  AA_REQUIRE(plan && name && workspace && ptr && ld, "aa_model_debug_tap: null argument");
  std::string n(name);
  int with_forces = 0;
  if (n.size() > 2 && n.compare(n.size() - 2, 2, "+f") == 0) {  // layout of a step that computed forces
    with_forces = 1;
    n.resize(n.size() - 2);
  }
  Workspace w = layout_workspace(plan, N, E, with_forces);
  const char* base = static_cast<const char*>(workspace);
  if (n == "edge_attrs") {
    *ptr = base + w.sh;
    *ld = plan->D;
  } else if (n == "edge_embedding") {
    *ptr = base + w.emb;
    *ld = plan->cfg.num_scalar;
  } else if (n == "edge_features") {
    *ptr = base + w.fcat;
    *ld = plan->SL1;
  } else if (n == "emb0") {
    *ptr = base + w.emb0;
    *ld = plan->cfg.embed_dim;
  } else if (n == "vec") {  // [E,4] unit vector, length
    *ptr = base + w.vec;
    *ld = 4;
  } else if (n == "dvec" && with_forces) {  // [E,4] dE/dr_e
    *ptr = base + w.dvec;
    *ld = 4;
  } else if (n == "gsh_env0" && with_forces && plan->pipe.channel_minor() && plan->pipe.tp_op < 0 && plan->cfg.num_layers >= 1) {
    // [E,D] layer-0 env slab of d Y (slot 1 of g_sh): tp_mom_bwd_first, or the last reverse chain under StepPlan::mom0_in_chain
    *ptr = base + w.g_sh + size_t(E) * plan->D * plan->esize();
    *ld = plan->D;
  } else if (n == "trev" && with_forces && plan->pipe.embed_fused) {  // [E,8] d E / d (the 8 basis functions), last reverse chain
    *ptr = base + w.trev;
    *ld = 8;
  } else {
    return fail(AA_ERR_INVALID, "aa_model_debug_tap: unknown tap");
  }
  return int(*ld);
}

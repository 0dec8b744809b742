// Developer / test switches of a stream-set's launch plan: the one table of them, the typed struct they resolve to, and the resolver.
// Host only (no HIP header: tests/test_plan_switches_cpu.py compiles it with g++).
//
// A switch is named in conan_streams_opts.dev_plan ("NAME=value;NAME"; a bare NAME means NAME=1) or, in `make DEV=1` builds only
// (CONAN_DEV_SWITCHES), in the environment as CONAN_<NAME>; the text wins.  conan_streams_create_opts resolves both ONCE, before it
// allocates anything: the launch path reads the fields of conan_streams::sw and nothing else, and a variable changed after creation
// has no effect.  The shipped library reads no environment variable and rejects the dev-only rows as unknown names.
#pragma once
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace plan {

constexpr int kMaxUps = 8;      // CONAN_MAX_UPS (streams.h asserts it)
#ifdef CONAN_DEV_SWITCHES
constexpr bool kDevBuild = true;
#else
constexpr bool kDevBuild = false;
#endif

struct PlanSwitches {      // (resolve() sets every field from its row's default)
  int reserve_cus, front_custride, emf_custride, front_prio, emf_cluster;
  bool rowconv, rb_nomerge, rb_nolimb, rb_unfused, rb_fused, rb_pair, rb_nopair, fenced, emf_unfused, no_tall;
  int rp_min_slots, tall_maxt;
  bool dec_mega, mega_narrow, mega_nol2, mega_layout_member_fastest;
  int mega_grid, mega_gs;
  int ups_cfg[kMaxUps];
  // dev-only rows
  bool no_tailsplit, mega_stamps, mega_xcd_pad, mega_noffn, rc_noksplit, emf_hold;
  int sk_min, cl_shape, rc_wide_min, skip_stage;
};

// How a row turns its value text into its field.  The spellings are the ones the read sites had grown; tests and scripts depend on
// them (NO_TALL=0 switches the feature, FENCED=2 does not), so they are recorded here, not tidied.
enum class Rule { Present, First1, FirstNot0, FirstM, Int, IntPositive, IntGroup, IntNonEmpty, CfgList };
inline const char* rule_text(Rule r) {
  switch (r) {
    case Rule::Present: return "on when named, whatever the value";
    case Rule::First1: return "on when the value starts with `1`";
    case Rule::FirstNot0: return "off when the value starts with `0`";
    case Rule::FirstM: return "on when the value starts with `m`";
    case Rule::Int: return "`atoi` of the value";
    case Rule::IntPositive: return "`atoi` of the value when it is above 0, else ignored";
    case Rule::IntGroup: return "`atoi` of the value when it is 4, 8 or 16, else ignored";
    case Rule::IntNonEmpty: return "`atoi` of the value when it is not empty, else ignored";
    case Rule::CfgList: return "comma list, entry i = `atoi` for upsampler i; an empty entry forces nothing";
  }
  return "?";
}

struct Row {
  const char* name;
  Rule rule;
  int def;               // bools: 0 / 1; CfgList: every entry
  bool dev_only;         // exists in `make DEV=1` builds only: the shipped library rejects the name as unknown
  bool PlanSwitches::*b;
  int PlanSwitches::*i;
  const char* what;
};
constexpr Row flag(const char* name, Rule rule, int def, bool dev_only, bool PlanSwitches::*f, const char* what) { return {name, rule, def, dev_only, f, nullptr, what}; }
constexpr Row num(const char* name, Rule rule, int def, bool dev_only, int PlanSwitches::*f, const char* what) { return {name, rule, def, dev_only, nullptr, f, what}; }

using P = PlanSwitches;
constexpr Row kRows[] = {
    num("RESERVE_CUS", Rule::Int, 0, false, &P::reserve_cus, "CUs the pipelined vocoder's persistent launches leave to the front-end streams"),
    flag("ROWCONV", Rule::FirstNot0, 1, false, &P::rowconv, "frame-rate decoder layers through rowconv.hip (off: conv_mfma + LayerNorm launches)"),
    flag("RB_NOMERGE", Rule::Present, 0, false, &P::rb_nomerge, "last-dilation ResBlock launches as separate branches + mean_act"),
    flag("RB_NOLIMB", Rule::Present, 0, false, &P::rb_nolimb, "arith = auto resolves to f32 (never overrides an explicit request)"),
    flag("FENCED", Rule::First1, 0, false, &P::fenced, "release / acquire fences around the inter-workgroup hand-offs too"),
    flag("DEC_MEGA", Rule::FirstNot0, 1, false, &P::dec_mega, "the decoder step as one persistent launch (off: separate launches)"),
    num("MEGA_GRID", Rule::IntPositive, 0, false, &P::mega_grid, "workgroups of the decoder launch, clamped to the CU count (0: 128, not clamped)"),
    num("FRONT_CUSTRIDE", Rule::Int, 0, false, &P::front_custride, "s >= 2: the pipelined decoder's stream uses CUs i % s == 0 only, and DEC_MEGA is off"),
    num("EMF_CUSTRIDE", Rule::Int, 0, false, &P::emf_custride, "s >= 2: the pipelined Emformer's stream uses CUs i % s == 0 only, and it forms no clusters"),
    num("MEGA_GS", Rule::IntGroup, 8, false, &P::mega_gs, "workgroups per group of the multi-tile decoder launch"),
    flag("MEGA_NARROW", Rule::FirstNot0, 1, false, &P::mega_narrow, "narrow layers of multi-tile decoder launches as K-split 16-column strips"),
    flag("MEGA_NOL2", Rule::Present, 0, false, &P::mega_nol2, "multi-tile decoder launch: agent-scope hand-offs even for groups on one XCD"),
    flag("MEGA_LAYOUT", Rule::FirstM, 0, true, &P::mega_layout_member_fastest, "m: member-fastest groups - UNSAFE, a GPU memory fault is on record (profiles/r6_stress_layout.txt)"),
    num("FRONT_PRIO", Rule::Int, 0, false, &P::front_prio, "1 / -1: the pipelined front-end streams at the highest / lowest priority"),
    flag("RB_UNFUSED", Rule::Present, 0, false, &P::rb_unfused, "no fused ResBlock tile pass and no pair kernel in any stage"),
    flag("RB_FUSED", Rule::Present, 0, false, &P::rb_fused, "the fused ResBlock tile pass in the wide stages at any slot count"),
    flag("RB_PAIR", Rule::Present, 0, false, &P::rb_pair, "limb stream-sets keep the pair kernel in the wide first stage"),
    flag("RB_NOPAIR", Rule::Present, 0, false, &P::rb_nopair, "no pair kernel in the wide first stage"),
    num("RP_MIN_SLOTS", Rule::Int, 16, false, &P::rp_min_slots, "fewest slots at which the wide first stage takes the pair kernel"),
    num("UPS_CFG", Rule::CfgList, -1, false, nullptr, "tile configuration (ConvCfg index) forced on upsampler i; out-of-range entries are ignored"),
    num("EMF_CLUSTER", Rule::Int, 0, false, &P::emf_cluster, "workgroups per stream group of the fused Emformer step (0: chosen per launch)"),
    flag("EMF_UNFUSED", Rule::First1, 0, false, &P::emf_unfused, "the Emformer step as separate launches"),
    flag("NO_TALL", Rule::Present, 0, false, &P::no_tall, "no split-K limb GEMM (conv_tall.hip) for the upsamplers"),
    num("TALL_MAXT", Rule::Int, 32, false, &P::tall_maxt, "most rows per slot at which conv_tall is taken"),
    flag("NO_TAILSPLIT", Rule::Present, 0, true, &P::no_tailsplit, "conv_mfma: no split-K tail for tile counts that are no multiple of the CU count"),
    num("SK_MIN", Rule::Int, 12, true, &P::sk_min, "conv_mfma 32-row tiles: fewest K-steps a split must take off the critical path"),
    flag("MEGA_STAMPS", Rule::Present, 0, true, &P::mega_stamps, "per-operator clock stamps of the last decoder launch, printed at destruction"),
    flag("MEGA_XCD_PAD", Rule::Present, 0, true, &P::mega_xcd_pad, "pipelined single-tile decoder launches keep their padded LDS size"),
    flag("MEGA_NOFFN", Rule::Present, 0, true, &P::mega_noffn, "multi-tile decoder launch: feed-forward layers as two operators"),
    num("CL_SHAPE", Rule::IntNonEmpty, -1, true, &P::cl_shape, "conv_limb tile shape index forced on every launch it fits"),
    flag("RC_NOKSPLIT", Rule::Present, 0, true, &P::rc_noksplit, "rowconv: no K split over the waves for single-tile launches"),
    num("RC_WIDE_MIN", Rule::Int, 1024, true, &P::rc_wide_min, "rowconv: fewest output columns for the 4-column-tile build"),
    num("SKIP_STAGE", Rule::Int, 0, true, &P::skip_stage, "timing only, results are garbage: bit 0 skips the pipelined Emformer launch, bit 1 the decoder's"),
    flag("EMF_HOLD", Rule::Present, 0, true, &P::emf_hold, "pipelined Emformer of step t waits for the vocoder of step t-2 to pass its wide first stage"),
};
constexpr int kNumRows = (int)(sizeof(kRows) / sizeof(kRows[0]));

// set the row's field from value text `v` (null: the row's default)
inline void apply(const Row& r, const char* v, PlanSwitches& sw) {
  int x = r.def;
  if (v) {
    const int n = atoi(v);
    switch (r.rule) {
      case Rule::Present: x = 1; break;
      case Rule::First1: x = v[0] == '1'; break;
      case Rule::FirstNot0: x = v[0] != '0'; break;
      case Rule::FirstM: x = v[0] == 'm'; break;
      case Rule::Int: x = n; break;
      case Rule::IntPositive: if (n > 0) x = n; break;
      case Rule::IntGroup: if (n == 4 || n == 8 || n == 16) x = n; break;
      case Rule::IntNonEmpty: if (*v) x = n; break;
      case Rule::CfgList: break;
    }
  }
  if (r.rule == Rule::CfgList) {
    for (int u = 0; u < kMaxUps; ++u) {
      sw.ups_cfg[u] = r.def;
      if (!v) continue;
      if (*v && *v != ',') sw.ups_cfg[u] = atoi(v);
      while (*v && *v != ',') ++v;
      v = *v ? v + 1 : nullptr;
    }
  } else if (r.b) sw.*r.b = x != 0;
  else sw.*r.i = x;
}

using EnvLookup = const char* (*)(const char*);
inline const char* process_env(const char* name) {
#ifdef CONAN_DEV_SWITCHES
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// The only reader of dev_plan text and (DEV builds) of the environment.  Throws std::invalid_argument for a name that is in no row of
// this build's table.
inline PlanSwitches resolve(const char* text, EnvLookup env = process_env) {
  PlanSwitches sw{};
  bool named[kNumRows] = {};
  for (const Row& r : kRows) apply(r, nullptr, sw);
  const std::string t(text ? text : "");
  for (size_t p = 0; p < t.size();) {
    size_t q = t.find(';', p);
    if (q == std::string::npos) q = t.size();
    std::string item = t.substr(p, q - p);
    p = q + 1;
    while (!item.empty() && item.front() == ' ') item.erase(item.begin());
    while (!item.empty() && item.back() == ' ') item.pop_back();
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    const std::string name = item.substr(0, eq), value = eq == std::string::npos ? "1" : item.substr(eq + 1);
    int k = 0;
    while (k < kNumRows && (name != kRows[k].name || (kRows[k].dev_only && !kDevBuild))) ++k;
    if (k == kNumRows) throw std::invalid_argument("conan_streams_opts.dev_plan: unknown switch '" + name + "'");
    apply(kRows[k], value.c_str(), sw);      // (a name given twice: the last one holds, from the row's default)
    named[k] = true;
  }
#ifdef CONAN_DEV_SWITCHES
  for (int k = 0; k < kNumRows; ++k) {
    const char* v = named[k] ? nullptr : env((std::string("CONAN_") + kRows[k].name).c_str());
    if (v) apply(kRows[k], v, sw);
  }
#else
  (void)env; (void)named;
#endif
  return sw;
}

// workgroups of the decoder's persistent launch on a device of num_cu CUs
inline int mega_grid(const PlanSwitches& sw, int num_cu) { return sw.mega_grid > 0 ? (sw.mega_grid < num_cu ? sw.mega_grid : num_cu) : 128; }

}  // namespace plan

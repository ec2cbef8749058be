// engine_calib.cpp — load-time precision calibration: measures the mixed-precision split set on the weights that are loaded and widens
// it (re-planning the engine for every trial) until the final maps are inside the target.
#include "engine_internal.h"

extern "C" {

// ---- load-time precision calibration ----------------------------------------------------------------
// The default split set of RTP_PREC_MIXED was chosen on one synthetic weight set.  Trained weights arrive through
// CopyTrainedLayersFrom (net.cpp:750-803) with another spectrum; this measures the set on the weights that are LOADED:
//   reference  = the same frames through RTP_PREC_F16X3 (every layer as hi + lo fp16 pairs: 1e-5 of the map maximum vs fp32),
//   candidate  = the current mixed plan;  err = max |candidate - reference| / max |reference|  over the final maps.
// While err > target, every layer group that is not split yet is tried on top of the current set and the one that lowers the
// error most is promoted; when every group is in and the error still exceeds the target the engine falls back to F16X3.
int rtp_calibrate_precision(rtp_engine* e, const float* frames_host, int nframes, float target, char* rules_out, size_t rules_len,
                            float* err_before, float* err_after) {
  // (no process-wide lock across this function: every re-plan and every tap below takes g_sync_mutex for its own captures / synchronous
  // calls, so other engines of the process — rtpose.bin --num_gpu N --calibrate K — interleave with the trials instead of queueing behind
  // the dozens of seconds a calibration can take)
  int rc;
  if ((rc = need_idle(e))) return rc;
  if ((rc = need_weights(e))) return rc;
  if (e->mode == RTP_PREC_F16X3 && e->calib_fell_back) {   // an earlier calibration ended in the parity-grade mode: nothing is left to adjust
    if (err_before) *err_before = 0.f;
    if (err_after) *err_after = 0.f;
    if (rules_out && rules_len) snprintf(rules_out, rules_len, "@f16x3");
    e->calib_report += "; called again: already RTP_PREC_F16X3 (every layer runs three fp16 passes), nothing to adjust";
    return RTP_OK;
  }
  if (e->mode != RTP_PREC_MIXED) return fail(e, RTP_EINVAL, "rtp_calibrate_precision adjusts the split set of RTP_PREC_MIXED (engine precision is %d)", e->mode);
  if (nframes < 1 || nframes > 64) return fail(e, RTP_EINVAL, "calibration frames %d out of range [1, 64]", nframes);
  if (!(target > 0.f)) target = 0.7e-3f;
  const size_t in_floats = (size_t)e->N * 3 * e->cfg.net_h * e->cfg.net_w;
  const size_t low_floats = (size_t)e->N * e->plan.heat_channels * e->plan.low_h * e->plan.low_w;
  std::vector<float> synth;
  if (!frames_host) {  // what process_and_pad_image makes of a u8 frame: v / 256 - 0.5 (rtpose.cpp:259), seeded
    synth.resize(in_floats * nframes);
    uint64_t st = 0x9E3779B97F4A7C15ull ^ e->cfg.synthetic_seed;
    for (float& v : synth) { st = st * 6364136223846793005ull + 1442695040888963407ull; v = (float)((st >> 56) & 0xff) / 256.0f - 0.5f; }
    frames_host = synth.data();
  }
  std::vector<float> ref(low_floats * nframes), got(low_floats);
  auto run = [&](const float* x, float* out) { return rtp_forward_heatmaps(e, x, out); };
  const std::string base_rules = e->split_rules;
  // a failure half way (a trial plan that does not fit the device, a HIP error) must not leave the caller with a one-context trial engine:
  // put the plan it came with back (best effort) and report the original error
  auto bail = [&](int code) {
    const std::string msg = e->err;
    if (replan(e, RTP_PREC_MIXED, base_rules, false) != RTP_OK) {
      // the restore failed too (e.g. the same out-of-memory condition): the engine has NO plan.  Mark it: every entry point that would
      // touch a context reports RTP_EHIP instead of dereferencing an empty vector; rtp_engine_destroy still works.
      drop_plan(e);
      e->broken = true;
      e->err = msg + " (and the engine's previous plan could not be restored: the engine is unusable, destroy it)";
      return code;
    }
    e->err = msg;
    return code;
  };
  // reference maps
  if ((rc = replan(e, RTP_PREC_F16X3, base_rules, true))) return bail(rc);
  for (int f = 0; f < nframes; ++f)
    if ((rc = run(frames_host + (size_t)f * in_floats, ref.data() + (size_t)f * low_floats))) return bail(rc);
  double norm = 0;
  for (float v : ref) norm = std::max(norm, (double)std::fabs(v));
  if (!(norm > 0) || !std::isfinite(norm)) {
    if (bail(RTP_ERANGE) && e->broken) return RTP_ERANGE;
    return fail(e, RTP_ERANGE, "calibration: the reference maps are %s (weights / frames out of range for fp16 storage?)", norm > 0 ? "not finite" : "all zero");
  }
  auto measure = [&](double* err) -> int {
    double m = 0;
    for (int f = 0; f < nframes; ++f) {
      int r2 = run(frames_host + (size_t)f * in_floats, got.data());
      if (r2) return r2;
      const float* rf = ref.data() + (size_t)f * low_floats;
      for (size_t i = 0; i < low_floats; ++i) {
        const double d = std::fabs((double)got[i] - (double)rf[i]);
        m = (d == d) ? std::max(m, d) : 1e30;   // NaN counts as unbounded
      }
    }
    *err = m / norm;
    return RTP_OK;
  };
  std::ostringstream rep;
  std::string rules = base_rules;
  double err = 0;
  if ((rc = replan(e, RTP_PREC_MIXED, rules, true))) return bail(rc);
  if ((rc = measure(&err))) return bail(rc);
  if (err_before) *err_before = (float)err;
  rep << "target " << target << "; frames " << nframes << "; set \"" << rules << "\" err " << err;
  // the layer groups a rule can name: trunk blocks by their "convN_" prefix, stage 1, the refinement stages (from the MIXED plan's flags)
  std::vector<std::string> all_groups;
  {
    auto add = [&](const std::string& g) { if (std::find(all_groups.begin(), all_groups.end(), g) == all_groups.end()) all_groups.push_back(g); };
    for (auto& c : e->plan.convs) {
      const size_t st = c.name.find("_stage");
      if (st != std::string::npos) { size_t en = st + 6; while (en < c.name.size() && isdigit((unsigned char)c.name[en])) ++en; add("*" + c.name.substr(st, en - st) + "_"); }
      else { const size_t us = c.name.find('_'); add(us == std::string::npos ? c.name : c.name.substr(0, us + 1)); }
    }
  }
  auto in_group = [](const std::string& g, const ConvOp& c) { return g[0] == '*' ? c.name.find(g.substr(1)) != std::string::npos : c.name.compare(0, g.size(), g) == 0; };
  auto open_groups = [&](bool want_h8) {   // groups with a layer that is not fully split yet (stage 1) / that still runs an fp8 chunk (stage 2)
    std::vector<std::string> gs;
    for (auto& g : all_groups) {
      bool open = false;
      for (auto& c : e->plan.convs) if (in_group(g, c) && (want_h8 ? c.h8 : !(c.split_w && (c.split_a || c.first)))) open = true;
      if (open) gs.push_back(g);
    }
    return gs;
  };
  // stage 1: promote un-split groups, the one that lowers the error most first
  std::vector<std::string> groups = open_groups(false);
  while (err > target && !groups.empty()) {
    int best = -1;
    double best_err = 1e300;
    for (size_t g = 0; g < groups.size(); ++g) {
      double eg = 0;
      if ((rc = replan(e, RTP_PREC_MIXED, rules + "," + groups[g], true))) return bail(rc);
      if ((rc = measure(&eg))) return bail(rc);
      rep << "; try +" << groups[g] << " -> " << eg;
      if (eg < best_err) { best_err = eg; best = (int)g; }
    }
    rules += "," + groups[best];
    rep << "; promote " << groups[best];
    groups.erase(groups.begin() + best);
    err = best_err;
  }
  // stage 2: every group is split and the target is still missed — the fp8 correction chunks are the limit (e4m3 operands: activations
  // beyond +-112 or rounding errors beyond their range saturate; 3 mantissa bits).  Groups switch to fp16 correction passes (":x"),
  // ranked by what the switch gains alone, applied cumulatively until the target holds.
  if (err > target) {
    if ((rc = replan(e, RTP_PREC_MIXED, rules, true))) return bail(rc);
    std::vector<std::string> hg = open_groups(true);
    std::vector<std::pair<double, std::string>> gain;
    for (auto& g : hg) {
      double eg = 0;
      if ((rc = replan(e, RTP_PREC_MIXED, rules + "," + g + ":x", true))) return bail(rc);
      if ((rc = measure(&eg))) return bail(rc);
      rep << "; try " << g << ":x -> " << eg;
      gain.push_back({eg, g});
    }
    std::sort(gain.begin(), gain.end());
    for (auto& ge : gain) {
      if (err <= target) break;
      rules += "," + ge.second + ":x";
      if ((rc = replan(e, RTP_PREC_MIXED, rules, true))) return bail(rc);
      if ((rc = measure(&err))) return bail(rc);
      rep << "; switch " << ge.second << ":x -> " << err;
    }
  }
  int final_mode = RTP_PREC_MIXED;
  if (err > target) {   // every layer runs three fp16 passes already where it can: the parity-grade mode for all of them
    final_mode = RTP_PREC_F16X3;
    rep << "; err " << err << " > target with every group switched: falling back to RTP_PREC_F16X3";
    err = 0;
  }
  if ((rc = replan(e, final_mode, final_mode == RTP_PREC_MIXED ? rules : base_rules, false))) return bail(rc);
  e->calib_fell_back = final_mode == RTP_PREC_F16X3;   // (rtp_get_split_layers then reports precision RTP_PREC_F16X3 next to the caller's own rule list: the rules do not apply in that mode)
  if (final_mode == RTP_PREC_MIXED && (rc = measure(&err))) return bail(rc);
  if (err_after) *err_after = (float)err;
  rep << "; final " << (final_mode == RTP_PREC_MIXED ? "mixed" : "f16x3") << " set \"" << rules << "\" err " << err;
  e->calib_report = rep.str();
  if (rules_out && rules_len) snprintf(rules_out, rules_len, "%s", final_mode == RTP_PREC_MIXED ? rules.c_str() : "@f16x3");
  return RTP_OK;
}
const char* rtp_calibration_report(const rtp_engine* e) { return e ? e->calib_report.c_str() : ""; }
// The split set in force (rule list of rtp_config.split_layers syntax) and the precision mode (a calibration may have changed both).
int rtp_get_split_layers(const rtp_engine* e, char* buf, size_t buflen, int* precision) {
  if (!e) return RTP_EINVAL;
  if (precision) *precision = e->mode;
  if (buf && buflen) {
    if (e->split_rules.size() + 1 > buflen) {   // never a silently truncated rule list: the receiver would build another plan
      buf[0] = 0;
      return fail(const_cast<rtp_engine*>(e), RTP_ERANGE, "rtp_get_split_layers: the rule list needs %zu bytes, the buffer has %zu", e->split_rules.size() + 1, buflen);
    }
    snprintf(buf, buflen, "%s", e->split_rules.c_str());
  }
  return RTP_OK;
}

}  // extern "C"

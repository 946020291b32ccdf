// K14: the host half of the three-launch evaluation.  Argument checks, the workspace layout and the argument blocks
// of eval.hip's kernels (prep / fix-up / finish, eval_abi.h) and of the rank GEMM that runs between them (sim.hip,
// through sim_abi.h): cmve_eval_ranks, the cmve_eval_batch_* family, cmve_eval_graph_* and the timing entries.
#include <algorithm>
#include <vector>

#include "eval_abi.h"
#include "sim_abi.h"

// Study knobs are compile-time only (make study NAME=x DEFS="-D..."): the product build reads no environment.
#ifndef CMVE_EVAL_DBG
#define CMVE_EVAL_DBG 0  // K14 kernel studies: 128 = per-block stamps (tools/eval_stamps.py, tools/batch_stamps.py)
#endif

using namespace cmve;

namespace {
struct EvalWs {
  size_t done, q_sgt, q_hi, q_lo, q_cnt, g_sgt, g_hi, g_lo, g_cnt, q_gt1, g_gt1, q_el, g_el, q_l8, g_l8, l3, cand,
      total;
};
// the lo8 planes: [n_pad, d_pad] bytes each side, the level-2 re-score's residuals (lo8_elem); l3: the level-3
// list (a count word, then EVAL_L3_CAP entries)
constexpr int EVAL_L3_CAP = 4096;
EvalWs eval_ws_layout(int64_t nq_pad, int64_t ng_pad, int64_t d_pad, int64_t cand_cap) {
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  EvalWs w;
  size_t o = 0;
  w.done = o;
  o = up(o + 2 * sizeof(unsigned) * cmve::EVAL_ARRIVAL_WORDS);
  w.q_sgt = o;
  o = up(o + 8 * (size_t)nq_pad);
  w.q_hi = o;
  o = up(o + 4 * (size_t)nq_pad);
  w.q_lo = o;
  o = up(o + 4 * (size_t)nq_pad);
  w.q_cnt = o;
  o = up(o + 4 * (size_t)nq_pad);
  w.g_sgt = o;
  o = up(o + 8 * (size_t)ng_pad);
  w.g_hi = o;
  o = up(o + 4 * (size_t)ng_pad);
  w.g_lo = o;
  o = up(o + 4 * (size_t)ng_pad);
  w.g_cnt = o;
  o = up(o + 4 * (size_t)ng_pad);
  w.q_gt1 = o;
  o = up(o + 4 * (size_t)nq_pad);
  w.g_gt1 = o;
  o = up(o + 4 * (size_t)ng_pad);
  w.q_el = o;
  o = up(o + 4 * (size_t)nq_pad);
  w.g_el = o;
  o = up(o + 4 * (size_t)ng_pad);
  w.q_l8 = o;
  o = up(o + (size_t)nq_pad * (size_t)d_pad);
  w.g_l8 = o;
  o = up(o + (size_t)ng_pad * (size_t)d_pad);
  w.l3 = o;
  o = up(o + 8 + 8 * (size_t)EVAL_L3_CAP);
  w.cand = o;
  o = up(o + 8 * (size_t)cand_cap);
  w.total = o;
  return w;
}
}  // namespace

static unsigned long long* g_eval_stamps = nullptr;
// kernel studies only (not in cmve.h): copy the last CMVE_EVAL_DBG & 128 stamps to the host
extern "C" int cmve_eval_debug_stamps(void* host, int64_t bytes) {
  CMVE_REQUIRE(g_eval_stamps && host, "cmve_eval_debug_stamps: no stamps (CMVE_EVAL_DBG & 128)");
  CMVE_HIP(hipDeviceSynchronize());
  CMVE_HIP(hipMemcpy(host, g_eval_stamps, std::min<int64_t>(bytes, sizeof(unsigned long long) * 4 * 1024 * 8),
                     hipMemcpyDeviceToHost));
  return CMVE_OK;
}

extern "C" int cmve_eval_workspace(const cmve_rows_t* q, const cmve_rows_t* g, int64_t cand_cap, int64_t* bytes) {
  CMVE_REQUIRE(q && g && bytes, "cmve_eval_workspace: NULL argument");
  CMVE_REQUIRE(cand_cap > 0, "cmve_eval_workspace: cand_cap must be > 0");
  *bytes = (int64_t)eval_ws_layout(q->n_pad, g->n_pad, q->d_pad, cand_cap).total;
  return CMVE_OK;
}

static cmve::EvalSide eval_side(cmve_rows_t* r, const int64_t* off, const int32_t* idx, char* ws, size_t o_sgt,
                                size_t o_hi, size_t o_lo, size_t o_cnt, size_t o_gt1, int64_t* ranks) {
  cmve::EvalSide s{};
  s.raw = r->raw;
  s.ld = r->raw_ld;
  s.n = r->n;
  s.n_pad = r->n_pad;
  s.vec = r->raw_dtype == CMVE_F32 ? rows_vec4((const float*)r->raw, r->d, r->raw_ld)
                                    : rows_vec4((const double*)r->raw, r->d, r->raw_ld);
  s.flags = r->flags;
  s.eps = r->eps;
  s.hi = r->hi;
  s.lo = r->lo;
  s.h16 = r->h16;
  s.inv = r->inv_norm;
  s.err_hi = r->err_hi;
  s.err_hilo = r->err_hilo;
  s.err_h16 = r->err_h16;
  s.err_max = r->err_max;
  s.off = off;
  s.idx = idx;
  s.sgt = (double*)(ws + o_sgt);
  s.thr_hi = (float*)(ws + o_hi);
  s.thr_lo = (float*)(ws + o_lo);
  s.cnt = (int32_t*)(ws + o_cnt);
  s.gt1 = off ? (int32_t*)(ws + o_gt1) : nullptr;
  s.ranks = ranks;
  return s;
}

// K14 at G256 sizes: the persistent rank kernel reads explicit thresholds, so they are written here by
// the rule the 2-stage / ring kernels apply in-kernel (sim_kernel's thr_of: the other set's err_max
// folded from the prep's shards, then gt_thr_kernel's directed rounding); one thread per row of either set
struct EvalThrSide {
  const double* sgt;
  const float* err;
  const unsigned* emax_other;
  float* hi;
  float* lo;
  int64_t n_pad;
};
__global__ __launch_bounds__(256) void eval_thr_kernel(EvalThrSide s0, EvalThrSide s1, int64_t d_pad, int mode) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool first = r < s0.n_pad;
  const EvalThrSide& s = first ? s0 : s1;
  if (!first) r -= s0.n_pad;
  if (!s.hi || r >= s.n_pad) return;
  unsigned m = 0u;
  for (int k = 0; k < EVAL_EMAX_SHARDS; ++k) m = max(m, s.emax_other[k]);
  const double E = score_error_bound((double)s.err[r], (double)__uint_as_float(m), d_pad, mode);
  const double sgt = s.sgt[r];  // NaN (no GT, padding) or +inf (every GT NaN): never counted
  s.hi[r] = sgt < INFINITY ? f32_round_up(sgt + E) : INFINITY;
  s.lo[r] = sgt < INFINITY ? f32_round_down(sgt - E) : INFINITY;
}

// Everything of one K14 evaluation but its launches: argument checks, the workspace layout and the argument
// blocks of the prep / rank GEMM / fix-up / finish launches (cmve_eval_ranks launches them at once;
// cmve_eval_batch_create stores them in a device table)
struct EvalPlan {
  cmve::EvalSide sq, sg;
  cmve::EvalCommon c;
  SimArgs a;
  int qf, gf;
  bool paired, inline_fix;
};

static int eval_prepare(cmve_rows_t* q, cmve_rows_t* g, int32_t mode_flags, const int64_t* row_off,
                        const int32_t* row_idx, const int64_t* col_off, const int32_t* col_idx, void* ws,
                        int64_t ws_bytes, int64_t cand_cap, int64_t* out, const char* fn, EvalPlan& P,
                        bool batch = false) {
  const int32_t mode = mode_flags & 0xff;
  const bool paired_req = (mode_flags & CMVE_EVAL_PAIRED) != 0;
  CMVE_REQUIRE((mode_flags & ~(0xff | CMVE_EVAL_PAIRED)) == 0, "%s: unknown flags 0x%x", fn, mode_flags);
  int st = sim_validate_pair(q, g, mode, fn);
  if (st) return st;
  CMVE_REQUIRE(q->n > 0 && g->n > 0, "%s: both sets need rows", fn);
  CMVE_REQUIRE(q->raw && g->raw && q->inv_norm && g->inv_norm && q->err_hi && q->err_hilo && g->err_hi &&
                   g->err_hilo && q->err_max && g->err_max,
               "%s: packed-set arrays missing", fn);
  CMVE_REQUIRE(!((q->flags | g->flags) & CMVE_PACK_RAW), "%s: sets packed CMVE_PACK_RAW have no score bound", fn);
  CMVE_REQUIRE((q->raw_dtype == CMVE_F32 || q->raw_dtype == CMVE_F64) &&
                   (g->raw_dtype == CMVE_F32 || g->raw_dtype == CMVE_F64),
               "%s: raw rows must be F32 or F64", fn);
  CMVE_REQUIRE(q->raw_ld >= q->d && g->raw_ld >= g->d, "%s: raw_ld < d", fn);
  CMVE_REQUIRE((q->h16 == nullptr) == (q->err_h16 == nullptr) && (g->h16 == nullptr) == (g->err_h16 == nullptr),
               "%s: h16 and err_h16 go together", fn);
  CMVE_REQUIRE((row_off != nullptr) == (row_idx != nullptr) && (col_off != nullptr) == (col_idx != nullptr),
               "%s: GT offsets and indices go together", fn);
  CMVE_REQUIRE(row_off || col_off, "%s: no direction requested", fn);
  CMVE_REQUIRE(ws && out, "%s: NULL workspace / output", fn);
  const EvalWs w = eval_ws_layout(q->n_pad, g->n_pad, q->d_pad, cand_cap);
  CMVE_REQUIRE(cand_cap > 0 && ws_bytes >= (int64_t)w.total, "%s: workspace has %lld bytes, needs %lld", fn,
               (long long)ws_bytes, (long long)w.total);
  CandLayout l = cand_layout(g->n_pad, cand_cap);
  // one bucket per 64 x 64 output tile when the grid is small: each wave reserves its undecided-pair
  // slots on its own tile's counter (by 256 gallery rows a 1k x 1k evaluation has 4 counters, ~125
  // serialised returning atomics each); the fix-up walks them flat
  const int64_t nb_tiles = (q->n_pad >> 6) * (g->n_pad >> 6);
  const bool tile_buckets = nb_tiles <= FIXUP_MAX_BUCKETS_PER_XCD && cand_cap >= 8 * nb_tiles;
  if (tile_buckets) {
    l.nb = nb_tiles;
    l.cap_b = (cand_cap - nb_tiles) / nb_tiles;
  }
  CMVE_REQUIRE(l.cap_b > 0, "%s: cand_cap %lld cannot hold the %lld bucket counters", fn, (long long)cand_cap,
               (long long)l.nb);
  CMVE_REQUIRE((l.nb + 7) / 8 <= FIXUP_MAX_BUCKETS_PER_XCD, "%s: gallery set too large (%lld buckets)", fn,
               (long long)l.nb);
  char* base = (char*)ws;
  P.sq = eval_side(q, row_off, row_idx, base, w.q_sgt, w.q_hi, w.q_lo, w.q_cnt, w.q_gt1, out + CMVE_EVAL_OUT_HEAD);
  P.sg = eval_side(g, col_off, col_idx, base, w.g_sgt, w.g_hi, w.g_lo, w.g_cnt, w.g_gt1,
                   out + CMVE_EVAL_OUT_HEAD + q->n);
  cmve::EvalCommon& c = P.c;
  c = cmve::EvalCommon{};
  c.d = q->d;
  c.d_pad = q->d_pad;
  c.mode = mode;
  c.emax = (unsigned*)(base + w.done);
  uint64_t* cand = (uint64_t*)(base + w.cand);
  c.bucket = (unsigned long long*)cand;
  c.nb = l.nb;
  c.cap_b = l.cap_b;
  c.cand = cand;
  c.stats = out;
  constexpr bool stamps = (CMVE_EVAL_DBG & 128) != 0;  // kernel studies only (a study build)
  static unsigned long long* stamp_buf = nullptr;
  if (stamps && !stamp_buf) {
    CMVE_HIP(hipMalloc(&stamp_buf, sizeof(unsigned long long) * 4 * 1024 * 8));
    CMVE_HIP(hipMemset(stamp_buf, 0, sizeof(unsigned long long) * 4 * 1024 * 8));
  }
  c.stamps = stamps ? stamp_buf : nullptr;
  g_eval_stamps = c.stamps;
  P.qf = q->raw_dtype == CMVE_F64;
  P.gf = g->raw_dtype == CMVE_F64;
  if (paired_req)
    CMVE_REQUIRE(row_off && col_off && q->n == g->n && q->n_pad == g->n_pad,
                 "%s: CMVE_EVAL_PAIRED needs both directions and equal set sizes", fn);
  // the paired prep reads rows through the register path only (16-B pieces, d_pad <= 1024)
  P.paired = paired_req && P.sq.vec && P.sg.vec && q->d_pad <= 1024;
  SimArgs& a = P.a;
  a = sim_make_args(q, g, mode);
  // thresholds derived in the GEMM from the prep's GT scores and per-row bounds (row_hi / col_hi only
  // mark the directions that are on)
  a.thr_gt = !sim_uses_phased(q->n_pad, g->n_pad);
  a.q_err = mode_err(q, mode);
  a.g_err = mode_err(g, mode);
  a.q_emax = c.emax + (0 * 3 + mode_slot(mode)) * cmve::EMAX_SHARDS;
  a.g_emax = c.emax + (1 * 3 + mode_slot(mode)) * cmve::EMAX_SHARDS;
  if (row_off) {
    a.row_hi = P.sq.thr_hi;
    a.row_lo = P.sq.thr_lo;
    a.row_sgt = P.sq.sgt;
    a.row_cnt = P.sq.cnt;
  }
  if (col_off) {
    a.col_hi = P.sg.thr_hi;
    a.col_lo = P.sg.thr_lo;
    a.col_sgt = P.sg.sgt;
    a.col_cnt = P.sg.cnt;
  }
  sim_set_cand(a, g, cand, cand_cap, out + 10);  // (the epilogue never writes cand_count)
  a.bucket_cnt = (unsigned long long*)cand;  // the evaluation's layout (l: per-tile buckets when small)
  a.cand = (unsigned long long*)(cand + l.nb);
  a.cap_b = l.cap_b;
  a.tile_buckets = tile_buckets;
  a.nbn64 = (int)(g->n_pad >> 6);
  if (a.thr_gt) {  // (the 2-stage / ring kernels; the persistent G256 kernel keeps every undecided pair)
    a.row_gt1 = P.sq.gt1;
    a.col_gt1 = P.sg.gt1;
  }
  // G64 (1k-A scale): the rank GEMM re-scores its own undecided pairs (no list, no fix-up launch)
  P.inline_fix = a.thr_gt && sim_uses_g64(q->n_pad, g->n_pad);
  // level-2 re-score from the fp16 + 8-bit residual planes: the F16 mode whose prep runs the register path (the
  // only one that writes lo8: 16-B row pieces, d_pad <= 1024, both sides).  Level 2 runs inside the rank GEMM, which
  // counts the pairs it leaves for level 3 (out[12]).  ONE evaluation (cmve_eval_ranks, its graphs) re-scores those
  // in the GEMM too (its ~4 pairs cost the GEMM ~0.7 us and spare the finish its fp64 round trip: 32.5 -> 31.4 us
  // back to back); batches list them for the finish (in a chained run it rides in the next prep launch).  The forms
  // that were measured and dropped (a fix-up launch, fp64 only, a listed level 3 for one evaluation):
  // profiles/STUDIES.md
  const bool l2 = P.inline_fix && mode == CMVE_SIM_F16 && P.sq.vec && P.sg.vec && q->d_pad <= 1024;
  if (l2) {
    P.sq.lo8 = (uint8_t*)(base + w.q_l8);
    P.sg.lo8 = (uint8_t*)(base + w.g_l8);
    P.sq.err_lo8 = (float*)(base + w.q_el);
    P.sg.err_lo8 = (float*)(base + w.g_el);
    a.q_lo8 = P.sq.lo8;
    a.g_lo8 = P.sg.lo8;
    a.q_el = P.sq.err_lo8;
    a.g_el = P.sg.err_lo8;
    c.l3_count = (unsigned*)(base + w.l3);
    c.l3 = (uint64_t*)(base + w.l3 + 8);
    c.l3_cap = batch ? EVAL_L3_CAP : 0;  // (0: the finish re-scores nothing; its count still reaches out[12])
    a.l3_count = c.l3_count;
    a.l3 = batch ? (unsigned long long*)c.l3 : nullptr;
    a.l3_cap = c.l3_cap;
  }
  if (P.inline_fix) {  // the GEMM re-scores its undecided pairs: no list, never an overflow
    a.fix_inline = 1;
    a.q_f64 = P.qf;
    a.g_f64 = P.gf;
    a.q_raw = q->raw;
    a.g_raw = g->raw;
    a.q_ld = q->raw_ld;
    a.g_ld = g->raw_ld;
    a.d = q->d;
    a.q_inv = q->inv_norm;
    a.g_inv = g->inv_norm;
    c.fix_inline = 1;
  }
  a.dbg_stamps = c.stamps ? c.stamps + 3 * 1024 * 8 : nullptr;
  return CMVE_OK;
}

extern "C" int cmve_eval_ranks(cmve_handle_t h, cmve_rows_t* q, cmve_rows_t* g, int32_t mode_flags,
                               const int64_t* row_off, const int32_t* row_idx, const int64_t* col_off,
                               const int32_t* col_idx, void* ws, int64_t ws_bytes, int64_t cand_cap, int64_t* out,
                               int32_t timing_slot) {
  CMVE_REQUIRE(h, "cmve_eval_ranks: NULL handle");
  CMVE_REQUIRE(timing_slot >= -1 && timing_slot < CMVE_EVAL_TIMING_SLOTS, "cmve_eval_ranks: bad timing slot");
  EvalPlan P;
  int st = eval_prepare(q, g, mode_flags, row_off, row_idx, col_off, col_idx, ws, ws_bytes, cand_cap, out,
                        "cmve_eval_ranks", P);
  if (st) return st;
  const int32_t mode = mode_flags & 0xff;
  hipEvent_t* ev = nullptr;
  hipEvent_t* kev = nullptr;
  if (timing_slot >= 0) {
    ev = h->eval_ev[timing_slot];
    for (int k = 0; k < 4; ++k)
      if (!ev[k]) CMVE_HIP(hipEventCreate(&ev[k]));
    kev = h->eval_kev[timing_slot];
    for (int k = 0; k < 8; ++k)
      if (!kev[k]) CMVE_HIP(hipEventCreate(&kev[k]));
  }
  auto arm = [&](int k) {  // the next launch's own start / stop (cmve::launch)
    if (kev) cmve::g_launch_ev = cmve::LaunchEv{kev[2 * k], kev[2 * k + 1]};
  };
  hipStream_t s = h->stream;
  if (ev) CMVE_HIP(hipEventRecord(ev[0], s));
  arm(0);
  st = cmve::launch_eval(P.sq, P.sg, P.c, P.qf, P.gf, P.paired ? 3 : 0, s);
  if (st) return st;
  if (ev) CMVE_HIP(hipEventRecord(ev[1], s));
  const SimArgs& a = P.a;
  if (!a.thr_gt) {
    EvalThrSide t0{a.row_sgt, a.q_err, a.g_emax, row_off ? P.sq.thr_hi : nullptr, P.sq.thr_lo, q->n_pad};
    EvalThrSide t1{a.col_sgt, a.g_err, a.q_emax, col_off ? P.sg.thr_hi : nullptr, P.sg.thr_lo, g->n_pad};
    const int64_t nthr = q->n_pad + g->n_pad;
    hipLaunchKernelGGL(eval_thr_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, t0, t1, q->d_pad,
                       (int)mode);
    st = check_launch("eval_thr_kernel");
    if (st) return st;
  }
  arm(1);
  st = launch_rank_gemm(a, q, g, mode, s);
  if (st) return st;
  if (ev) CMVE_HIP(hipEventRecord(ev[2], s));
  if (timing_slot >= 0) {
    h->eval_no_fix[timing_slot] = P.inline_fix;
    h->eval_chained[timing_slot] = false;
  }
  if (!P.inline_fix) {
    arm(2);
    st = cmve::launch_eval(P.sq, P.sg, P.c, P.qf, P.gf, 1, s);
    if (st) return st;
  }
  arm(3);
  st = cmve::launch_eval(P.sq, P.sg, P.c, P.qf, P.gf, 2, s);
  if (st) return st;
  if (ev) CMVE_HIP(hipEventRecord(ev[3], s));
  return CMVE_OK;
}

// ---- K14 batches: same-shaped evaluations (MSR-VTT-1kA-sized, the G64 inline fix-up geometry) in ONE set of
// three launches, each with a grid of (blocks of one evaluation) x (evaluations): a 1k x 1k evaluation's
// launches leave most of the chip idle, a batch fills it (every launch's argument blocks in a device table).
struct cmve_eval_batch {
  int count = 0;
  int qf = 0, gf = 0, mode = 0;
  bool paired = false;
  int64_t nq_pad = 0, ng_pad = 0;
  int bm = 64, bn = 64;           // the rank tile (sim_batch_geo_bm / _bn)
  cmve::EvalSide sq0, sg0;        // the shapes (the launch grids)
  cmve::EvalCommon c0;            // (the first evaluation's: which prep kernel applies)
  cmve::EvalItem* d_items = nullptr;
  SimArgs* d_args = nullptr;
  std::vector<void*> ws;          // the evaluations' workspaces and outputs: a chained run refuses a previous batch
  std::vector<void*> outs;        // sharing either (its finish runs in the same launch as this batch's prep)
  bool chainable = false;         // the specialised paired prep: the chained run fuses it with the previous finish
  bool pending = false;           // its last run was chained and its finish has not been enqueued yet ...
  hipStream_t pending_stream = nullptr;  // ... on this stream (the next chained run there, or cmve_eval_batch_finish)
};

extern "C" int cmve_eval_batch_create(int32_t count, cmve_rows_t* const* q, cmve_rows_t* const* g,
                                      int32_t mode_flags, const int64_t* row_off, const int32_t* row_idx,
                                      const int64_t* col_off, const int32_t* col_idx, void* const* ws,
                                      int64_t ws_bytes, int64_t cand_cap, int64_t* const* out,
                                      cmve_eval_batch_t* batch) {
  CMVE_REQUIRE(batch && q && g && ws && out && count >= 1 && count <= 65535,
               "cmve_eval_batch_create: NULL argument / count out of [1, 65535]");
  *batch = nullptr;
  std::vector<cmve::EvalItem> items((size_t)count);
  std::vector<SimArgs> args((size_t)count);
  EvalPlan P0;
  for (int i = 0; i < count; ++i) {
    EvalPlan P;
    const int st = eval_prepare(q[i], g[i], mode_flags, row_off, row_idx, col_off, col_idx, ws[i], ws_bytes,
                                cand_cap, out[i], "cmve_eval_batch_create", P, true);
    if (st) return st;
    CMVE_REQUIRE(P.inline_fix, "cmve_eval_batch_create: batches take the G64 geometry (fewer than 128 tiles of "
                               "128^2, e.g. 1,000 x 1,000) with the inline fix-up");
    if (P.c.stamps) {  // kernel studies (CMVE_EVAL_DBG & 128): the first evaluation's prep / finish blocks, and
                       // every evaluation's rank tiles while the stamp buffer's 1,024 tile slots last
      const int64_t per = (q[i]->n_pad / sim_batch_geo_bm(q[i]->n_pad)) *
                          (g[i]->n_pad / sim_batch_geo_bn(q[i]->n_pad, g[i]->n_pad, mode_flags & 0xff));
      P.a.dbg_stamps = (i + 1) * per <= 1024 ? P.c.stamps + 3 * 1024 * 8 + (size_t)i * per * 8 : nullptr;
      if (i > 0) P.c.stamps = nullptr;
    }
    if (i == 0) {
      P0 = P;
    } else {
      CMVE_REQUIRE(q[i]->n == q[0]->n && g[i]->n == g[0]->n && q[i]->n_pad == q[0]->n_pad &&
                       g[i]->n_pad == g[0]->n_pad && q[i]->d == q[0]->d && q[i]->d_pad == q[0]->d_pad &&
                       P.qf == P0.qf && P.gf == P0.gf && P.paired == P0.paired,
                   "cmve_eval_batch_create: evaluation %d differs in shape / dtype / pairing from the first", i);
      // the batch's launches pick their kernels (the specialised paired prep, the level-2 re-score)
      // from the first evaluation's plan: every evaluation must plan the same way -- e.g. a row-strided input whose
      // rows are not 16-B aligned takes no register prep and no residual plane, which the specialised prep would
      // still read and write through
      CMVE_REQUIRE(P.sq.vec == P0.sq.vec && P.sg.vec == P0.sg.vec && (P.sq.lo8 != nullptr) == (P0.sq.lo8 != nullptr) &&
                       (P.sg.lo8 != nullptr) == (P0.sg.lo8 != nullptr) &&
                       (P.c.l3_count != nullptr) == (P0.c.l3_count != nullptr),
                   "cmve_eval_batch_create: evaluation %d's inputs take another path than the first's (row alignment "
                   "or stride: every evaluation of a batch needs 16-B aligned rows if the first has them)", i);
      for (int j = 0; j < i; ++j)
        CMVE_REQUIRE(ws[j] != ws[i] && out[j] != out[i],
                     "cmve_eval_batch_create: evaluations %d and %d share a workspace or an output", j, i);
    }
    items[(size_t)i] = cmve::EvalItem{P.sq, P.sg, P.c};
    // (launch_geo fills these for a single launch)
    sim_geo_fill(P.a, q[i]->n_pad, g[i]->n_pad, sim_batch_geo_bm(q[i]->n_pad),
                 sim_batch_geo_bn(q[i]->n_pad, g[i]->n_pad, mode_flags & 0xff));
    args[(size_t)i] = P.a;
  }
  auto* b = new cmve_eval_batch;
  b->count = count;
  b->qf = P0.qf;
  b->gf = P0.gf;
  b->mode = mode_flags & 0xff;
  b->paired = P0.paired;
  b->nq_pad = q[0]->n_pad;
  b->ng_pad = g[0]->n_pad;
  b->bm = sim_batch_geo_bm(b->nq_pad);
  b->bn = sim_batch_geo_bn(b->nq_pad, b->ng_pad, b->mode);
  b->sq0 = P0.sq;
  b->sg0 = P0.sg;
  b->c0 = P0.c;
  b->ws.assign(ws, ws + count);
  b->outs.assign(out, out + count);
  // the fused chained launch runs the specialised PAIRED prep: a batch whose lists are no one-to-one pairing (run()
  // takes the general prep, phase 0) chains through the separate finish launch instead
  b->chainable = P0.paired && cmve::eval_batch_chainable(P0.sq, P0.sg, P0.c);
  hipError_t e = hipMalloc(&b->d_items, sizeof(cmve::EvalItem) * (size_t)count);
  if (e == hipSuccess) e = hipMalloc(&b->d_args, sizeof(SimArgs) * (size_t)count);
  if (e == hipSuccess)
    e = hipMemcpy(b->d_items, items.data(), sizeof(cmve::EvalItem) * (size_t)count, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b->d_args, args.data(), sizeof(SimArgs) * (size_t)count, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(b->d_items);
    (void)hipFree(b->d_args);
    delete b;
    CMVE_HIP(e);
  }
  *batch = b;
  return CMVE_OK;
}

// timing_slot >= 0: the three launches' own start / stop into that slot of h's ring (cmve_eval_kernel_timing:
// prep, rank GEMM, 0, finish -- durations of the whole batch's launches) and the event spans (cmve_eval_timing).
// A chained run's prep slot includes the previous batch's finish (fused into the prep launch, or its own launch)
static int eval_batch_run(cmve_handle_t h, cmve_eval_batch_t b, int32_t timing_slot, bool chained = false,
                          cmve_eval_batch_t prev = nullptr) {
  hipEvent_t* ev = nullptr;
  hipEvent_t* kev = nullptr;
  if (timing_slot >= 0) {
    ev = h->eval_ev[timing_slot];
    for (int k = 0; k < 4; ++k)
      if (!ev[k]) CMVE_HIP(hipEventCreate(&ev[k]));
    kev = h->eval_kev[timing_slot];
    for (int k = 0; k < 8; ++k)
      if (!kev[k]) CMVE_HIP(hipEventCreate(&kev[k]));
    h->eval_no_fix[timing_slot] = true;  // (a batch re-scores in its rank GEMM)
    h->eval_chained[timing_slot] = chained;
  }
  auto arm = [&](int k) {
    if (kev) cmve::g_launch_ev = cmve::LaunchEv{kev[2 * k], kev[2 * k + 1]};
  };
  hipStream_t s = h->stream;
  int st = CMVE_OK;
  const bool fused = chained && b->chainable;  // the prep and the previous batch's finish in one launch
  if (ev) CMVE_HIP(hipEventRecord(ev[0], s));
  if (chained && prev && !fused) {  // (not the specialised prep: the previous batch's finish as a launch of its own,
    // inside the prep's timing span; its own kernel events are not taken -- slot 0's kernel pair times the prep)
    st = cmve::launch_eval_batch(prev->sq0, prev->sg0, prev->c0, prev->d_items, prev->count, prev->qf, prev->gf, 2, s);
    if (st) return st;
  }
  arm(0);
  if (fused)
    st = cmve::launch_eval_batch_chained(b->sq0, b->sg0, b->c0, b->d_items, prev ? prev->d_items : nullptr, b->count,
                                         b->qf, b->gf, s);
  else
    st = cmve::launch_eval_batch(b->sq0, b->sg0, b->c0, b->d_items, b->count, b->qf, b->gf, b->paired ? 3 : 0, s);
  if (st) return st;
  if (ev) CMVE_HIP(hipEventRecord(ev[1], s));
  arm(1);
  st = launch_rank_gemm_batch(b->d_args, b->count, b->nq_pad, b->ng_pad, b->mode, b->bm, b->bn, s);
  if (st) return st;
  if (ev) CMVE_HIP(hipEventRecord(ev[2], s));
  if (!chained) {
    arm(3);
    st = cmve::launch_eval_batch(b->sq0, b->sg0, b->c0, b->d_items, b->count, b->qf, b->gf, 2, s);
    if (st) return st;
  }
  if (ev) CMVE_HIP(hipEventRecord(ev[3], s));
  return CMVE_OK;
}

extern "C" int cmve_eval_batch_run(cmve_handle_t h, cmve_eval_batch_t b, int32_t timing_slot) {
  CMVE_REQUIRE(h && b && b->d_items && b->d_args, "cmve_eval_batch_run: NULL handle / batch");
  CMVE_REQUIRE(timing_slot >= -1 && timing_slot < CMVE_EVAL_TIMING_SLOTS, "cmve_eval_batch_run: bad timing slot");
  CMVE_REQUIRE(!b->pending, "cmve_eval_batch_run: the batch's last chained run is not finished (chain it as the previous "
                            "batch of the next chained run, or call cmve_eval_batch_finish)");
  return eval_batch_run(h, b, timing_slot);
}

extern "C" int cmve_eval_batch_run_chained(cmve_handle_t h, cmve_eval_batch_t b, cmve_eval_batch_t prev,
                                           int32_t timing_slot) {
  CMVE_REQUIRE(h && b && b->d_items && b->d_args, "cmve_eval_batch_run_chained: NULL handle / batch");
  CMVE_REQUIRE(timing_slot >= -1 && timing_slot < CMVE_EVAL_TIMING_SLOTS,
               "cmve_eval_batch_run_chained: bad timing slot");
  CMVE_REQUIRE(!b->pending, "cmve_eval_batch_run_chained: the batch's last chained run is not finished yet");
  if (prev) {
    CMVE_REQUIRE(prev->d_items && prev != b, "cmve_eval_batch_run_chained: the previous batch is destroyed or the batch itself");
    CMVE_REQUIRE(prev->pending && prev->pending_stream == h->stream,
                 "cmve_eval_batch_run_chained: the previous batch has no chained run awaiting its finish on this stream");
    CMVE_REQUIRE(prev->count == b->count && prev->nq_pad == b->nq_pad && prev->ng_pad == b->ng_pad &&
                     prev->sq0.n == b->sq0.n && prev->sg0.n == b->sg0.n && prev->qf == b->qf && prev->gf == b->gf &&
                     prev->mode == b->mode && prev->paired == b->paired && prev->chainable == b->chainable,
                 "cmve_eval_batch_run_chained: the previous batch differs in shape from the batch");
    for (void* w : b->ws)
      CMVE_REQUIRE(std::find(prev->ws.begin(), prev->ws.end(), w) == prev->ws.end(),
                   "cmve_eval_batch_run_chained: the batch shares a workspace with the previous batch, whose finish "
                   "runs in the same launch as its prep");
    // the prep zeroes out[0, 13) while the previous finish adds its R@K counts / rank sums into its own out
    const uintptr_t span = sizeof(int64_t) * (uintptr_t)(CMVE_EVAL_OUT_HEAD + b->sq0.n + b->sg0.n);
    for (void* o : b->outs)
      for (void* po : prev->outs)
        CMVE_REQUIRE((uintptr_t)o + span <= (uintptr_t)po || (uintptr_t)po + span <= (uintptr_t)o,
                     "cmve_eval_batch_run_chained: the batch shares an output with the previous batch, whose finish "
                     "runs in the same launch as its prep");
  }
  const int st = eval_batch_run(h, b, timing_slot, true, prev);
  if (st) return st;
  if (prev) prev->pending = false;
  b->pending = true;
  b->pending_stream = h->stream;
  return CMVE_OK;
}

extern "C" int cmve_eval_batch_finish(cmve_handle_t h, cmve_eval_batch_t b) {
  CMVE_REQUIRE(h && b && b->d_items, "cmve_eval_batch_finish: NULL handle / batch");
  CMVE_REQUIRE(b->pending && b->pending_stream == h->stream,
               "cmve_eval_batch_finish: the batch has no chained run awaiting its finish on this stream");
  const int st = cmve::launch_eval_batch(b->sq0, b->sg0, b->c0, b->d_items, b->count, b->qf, b->gf, 2, h->stream);
  if (st) return st;
  b->pending = false;
  return CMVE_OK;
}

extern "C" int cmve_eval_batch_destroy(cmve_eval_batch_t b) {
  if (!b) return CMVE_OK;
  (void)hipFree(b->d_items);
  (void)hipFree(b->d_args);
  delete b;
  return CMVE_OK;
}

// The graph form: the four launches of one cmve_eval_ranks call captured once (their kernel arguments --
// every pointer and size -- are baked in) and replayed with one hipGraphLaunch per evaluation: the host
// side of an evaluation drops from four kernel launches to one graph launch.
struct cmve_eval_graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

extern "C" int cmve_eval_graph_create(cmve_handle_t h, cmve_rows_t* q, cmve_rows_t* g, int32_t mode,
                                      const int64_t* row_off, const int32_t* row_idx, const int64_t* col_off,
                                      const int32_t* col_idx, void* ws, int64_t ws_bytes, int64_t cand_cap, int64_t* out,
                                      cmve_eval_graph_t* graph) {
  CMVE_REQUIRE(h && graph, "cmve_eval_graph_create: NULL handle / output");
  *graph = nullptr;
  CMVE_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
  const int st = cmve_eval_ranks(h, q, g, mode, row_off, row_idx, col_off, col_idx, ws, ws_bytes, cand_cap, out,
                                 -1);  // (mode may carry CMVE_EVAL_PAIRED)
  hipGraph_t gr = nullptr;
  const hipError_t e = hipStreamEndCapture(h->stream, &gr);
  if (st) {  // (the argument check failed inside the capture: nothing was enqueued)
    if (gr) (void)hipGraphDestroy(gr);
    return st;
  }
  CMVE_HIP(e);
  auto* eg = new cmve_eval_graph;
  eg->graph = gr;
  const hipError_t ie = hipGraphInstantiate(&eg->exec, gr, nullptr, nullptr, 0);
  if (ie != hipSuccess) {
    (void)hipGraphDestroy(gr);
    delete eg;
    CMVE_HIP(ie);
  }
  *graph = eg;
  return CMVE_OK;
}

extern "C" int cmve_eval_graph_launch(cmve_handle_t h, cmve_eval_graph_t graph) {
  CMVE_REQUIRE(h && graph && graph->exec, "cmve_eval_graph_launch: NULL handle / graph");
  CMVE_HIP(hipGraphLaunch(graph->exec, h->stream));
  return CMVE_OK;
}

extern "C" int cmve_eval_graph_destroy(cmve_eval_graph_t graph) {
  if (!graph) return CMVE_OK;
  if (graph->exec) CMVE_HIP(hipGraphExecDestroy(graph->exec));
  if (graph->graph) CMVE_HIP(hipGraphDestroy(graph->graph));
  delete graph;
  return CMVE_OK;
}

extern "C" int cmve_eval_timing(cmve_handle_t h, int32_t slot, float* ms3) {
  CMVE_REQUIRE(h && ms3 && slot >= 0 && slot < CMVE_EVAL_TIMING_SLOTS, "cmve_eval_timing: bad argument");
  hipEvent_t* ev = h->eval_ev[slot];
  CMVE_REQUIRE(ev[0] && ev[3], "cmve_eval_timing: slot %d never recorded", slot);
  CMVE_HIP(hipEventSynchronize(ev[3]));
  for (int k = 0; k < 3; ++k) CMVE_HIP(hipEventElapsedTime(&ms3[k], ev[k], ev[k + 1]));
  return CMVE_OK;
}

extern "C" int cmve_eval_kernel_timing(cmve_handle_t h, int32_t slot, float* ms4) {
  CMVE_REQUIRE(h && ms4 && slot >= 0 && slot < CMVE_EVAL_TIMING_SLOTS, "cmve_eval_kernel_timing: bad argument");
  hipEvent_t* kev = h->eval_kev[slot];
  const bool chained = h->eval_chained[slot];  // (cmve_eval_batch_run_chained: the finish ran in the next run's prep)
  const int last = chained ? 3 : 7;  // (a chained run is a batch's: prep and rank GEMM only)
  CMVE_REQUIRE(kev[0] && kev[last], "cmve_eval_kernel_timing: slot %d never recorded", slot);
  CMVE_HIP(hipEventSynchronize(kev[last]));
  for (int k = 0; k < 4; ++k) {
    if ((k == 2 && h->eval_no_fix[slot]) || (k == 3 && chained)) {  // no fix-up launch (re-scored in the rank GEMM) /
      ms4[k] = 0.f;                                                  // the finish deferred to the next chained run
      continue;
    }
    CMVE_HIP(hipEventElapsedTime(&ms4[k], kev[2 * k], kev[2 * k + 1]));
  }
  return CMVE_OK;
}

// What the host side of a filtered count shares, whatever the filter (K19 / K21: the MFMA filter of l2_filter.hip;
// K22: the SAD filter of l1_filter.hip; K24: the same filter under jaccard, jaccard_filter.hip) -- every one of them
// promises cmve_pairwise_count's words:
//   FltLists / FltBand   the caller's lists and band list, as every entry, launch and kernel argument carries them
//   flt_check_lists      what every count entry asks of the lists (cmve_pairwise_count included)
//   flt_count_run        the host body: checks, memsets, NaN items, the filter's main launch, fix-up, resolve
// A filter supplies its own operands' checks and a main launch (K26, the cosine filter of cos_filter.hip, also its
// fix-up launch and, K27, its resolve launch: its canonical word is cos64, not a chain of pairwise_tile.h).  The two SAD filters share one kernel body and one
// epilogue (sad_count.h: the same tile, thread layout and occupancy under a small policy); l2f_main_kernel keeps an
// epilogue of its own (the same algorithm on another thread layout, at 256 VGPRs): written once as a force-inlined
// template it cost that kernel 6% (DESIGN s4).
#ifndef CMVE_FILTER_COUNT_H
#define CMVE_FILTER_COUNT_H
#include "l2_filter_tile.h"

namespace cmve {

// the lists of a count: per direction the CSR offsets, the items' fp64 score words, their number, the caller's n
// (the NaN items' words) and the positions (NULL: direction not asked for)
struct FltLists {
  const int64_t* row_off;
  const double* row_sc;
  int64_t row_items, row_n;
  int32_t* row_pos;
  const int64_t* col_off;
  const double* col_sc;
  int64_t col_items, col_n;
  int32_t* col_pos;
};

// the band list and the counters of a filtered count
struct FltBand {
  int2* band;
  int64_t cap;
  l2f_u64* stats;  // {decided, band found, band re-scored, overflow}
};

// what flt_count_run hands a filter's main launch beside the filter's own operands (l2f_main_kernel takes it as it
// is; the SAD count kernels keep a flat argument block whose common prefix sad_count_args fills from it)
struct FltArgs {
  int64_t na, nb;
  double alpha, beta;
  FltLists lists;
  FltBand band;
  int tiles_a, tiles_b;
};

// The lists as every count entry wants them (`name`: the entry, for the refusals).  On success a direction
// without items has neither items nor positions: every launch skips it.
static inline int flt_check_lists(const char* name, FltLists& l) {
  if (!l.row_pos) l.row_items = 0;
  if (!l.col_pos) l.col_items = 0;
  CMVE_REQUIRE(l.row_items >= 0 && l.col_items >= 0 && l.row_n >= 0 && l.col_n >= 0 && l.row_n < (1ll << 31) &&
                   l.col_n < (1ll << 31) && l.row_items < (1ll << 31) * 256 && l.col_items < (1ll << 31) * 256,
               "%s: bad counts (%lld, %lld items; n %lld, %lld)", name, (long long)l.row_items,
               (long long)l.col_items, (long long)l.row_n, (long long)l.col_n);
  CMVE_REQUIRE(!l.row_pos || (l.row_off && (l.row_sc || !l.row_items)), "%s: row lists missing", name);
  CMVE_REQUIRE(!l.col_pos || (l.col_off && (l.col_sc || !l.col_items)), "%s: column lists missing", name);
  if (!l.row_items) l.row_pos = nullptr;
  if (!l.col_items) l.col_pos = nullptr;
  return CMVE_OK;
}

// ---- the launches that do not depend on how the pairs were filtered (`metric` is CMVE_PW_L2 or CMVE_PW_L1 with fp64
// words, or CMVE_PW_JACCARD with float32 words; FltRows, the raw rows of both sides, is l2_filter_tile.h's) ----
// the NaN items' words of one direction (n_lists lists, the caller's n); l2_filter.hip
void l2f_nan_launch(hipStream_t st, const int64_t* off, const double* sc, int64_t n_lists, int64_t n, int32_t* pos);
// the band list's pairs on the canonical chain (returns at once on the device when the list overflowed); l2_filter.hip
void l2f_fixup_launch(hipStream_t st, int32_t metric, const FltRows& r, double alpha, double beta, const FltLists& l,
                      const FltBand& b);
// the overflow resolved on the device: zero the words, then cmve_pairwise_count's tiles, both gated on stats[3];
// l2_filter.hip
void l2f_resolve_launch(hipStream_t st, int32_t metric, const FltRows& r, double alpha, double beta, const FltLists& l,
                        const l2f_u64* stats);
// cmve_pairwise_count's counting tiles (pairwise_rank.hip) with the metric's score words, gated: a bounded grid whose blocks
// return at once when *gate is 0 and loop over the tiles otherwise.  pos must be zero where *gate is not.
void pwr_count_gated_launch(hipStream_t st, int32_t metric, const FltRows& r, double alpha, double beta,
                            const FltLists& l, const l2f_u64* gate);

// ---- the host body -------------------------------------------------------------------------------------------------------
// One filtered count on h's stream.  `name`: the entry (refusals), `label`: check_launch's; own_checks(): the
// entry's checks of its own operands, run where they always ran (after the scaling, before the lists);
// main_launch(st, args): the filter's main kernel over args.tiles_a x args.tiles_b blocks.  `resolve`: an
// overflowing list is resolved on the device.  fixup_launch(st, lists, band): the re-score of the band list on the
// entry's canonical chain -- l2f_fixup_launch with `metric` for the measures of pairwise_tile.h (the overload below),
// K26's own under cosine (cos_filter.hip, whose words are cos64's).  resolve_launch(st, lists, band): the launches
// that give an overflowed call its words, gated on band.stats[3] -- l2f_resolve_launch with `metric` for those
// measures (the overload below), K27's own under cosine.
template <typename Own, typename Main, typename Fix, typename Res>
static inline int flt_count_run(const char* name, const char* label, cmve_handle_t h, int32_t metric,
                                const FltRows& r, double alpha, double beta, FltLists l, void* ws, int64_t ws_bytes,
                                int64_t* stats, bool resolve, Own own_checks, Main main_launch, Fix fixup_launch,
                                Res resolve_launch) {
  CMVE_REQUIRE(alpha != 0.0 && std::isfinite(alpha) && std::isfinite(beta),
               "%s: alpha must be finite and non-zero, beta finite (%g, %g)", name, alpha, beta);
  if (int rc = own_checks()) return rc;
  if (int rc = flt_check_lists(name, l)) return rc;
  CMVE_REQUIRE(ws_bytes >= 0 && (ws || ws_bytes < 8), "%s: workspace missing", name);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "%s: workspace must be 8-byte aligned", name);
  const int64_t tiles_a = (r.na + L2F_BM - 1) / L2F_BM, tiles_b = (r.nb + L2F_BN - 1) / L2F_BN;
  CMVE_REQUIRE(tiles_a * tiles_b < (1ll << 31), "%s: too many tiles (%lld x %lld)", name, (long long)tiles_a,
               (long long)tiles_b);
  const hipStream_t st = h->stream;
  CMVE_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
  if (l.row_items + l.col_items == 0) return CMVE_OK;
  if (l.row_items) CMVE_HIP(hipMemsetAsync(l.row_pos, 0, sizeof(int32_t) * l.row_items, st));
  if (l.col_items) CMVE_HIP(hipMemsetAsync(l.col_pos, 0, sizeof(int32_t) * l.col_items, st));
  // the NaN items' words are the caller's n, whatever this call's own na / nb
  if (l.row_items && l.row_n && r.na) l2f_nan_launch(st, l.row_off, l.row_sc, r.na, l.row_n, l.row_pos);
  if (l.col_items && l.col_n && r.nb) l2f_nan_launch(st, l.col_off, l.col_sc, r.nb, l.col_n, l.col_pos);
  if (r.na == 0 || r.nb == 0) return check_launch(label);
  const FltBand band{(int2*)ws, ws_bytes / (int64_t)sizeof(int2), (l2f_u64*)stats};
  main_launch(st, FltArgs{r.na, r.nb, alpha, beta, l, band, (int)tiles_a, (int)tiles_b});
  if (band.cap > 0) fixup_launch(st, l, band);
  if (resolve) resolve_launch(st, l, band);
  return check_launch(label);
}

template <typename Own, typename Main>
static inline int flt_count_run(const char* name, const char* label, cmve_handle_t h, int32_t metric,
                                const FltRows& r, double alpha, double beta, FltLists l, void* ws, int64_t ws_bytes,
                                int64_t* stats, bool resolve, Own own_checks, Main main_launch) {
  return flt_count_run(name, label, h, metric, r, alpha, beta, l, ws, ws_bytes, stats, resolve, own_checks, main_launch,
                       [&](hipStream_t st, const FltLists& fl, const FltBand& fb) {
                         l2f_fixup_launch(st, metric, r, alpha, beta, fl, fb);
                       },
                       [&](hipStream_t st, const FltLists& fl, const FltBand& fb) {
                         l2f_resolve_launch(st, metric, r, alpha, beta, fl, fb.stats);
                       });
}

}  // namespace cmve
#endif

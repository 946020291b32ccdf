// K4 GEMM (sim.hip): the kernel's argument block and what the K14 host (api_eval.hip) uses of its launch side.
#pragma once
#include "cmve_internal.h"

namespace cmve {

struct SimArgs {
  const uint16_t* qhi;
  const uint16_t* qlo;
  const uint16_t* ghi;
  const uint16_t* glo;
  int64_t ldk;  // d_pad
  int nq, ng;
  int nblk_m, nblk_n;
  int nk;   // K-tiles of the MFMA loop (split-bf16: 3 x nk0, see plane_of)
  int nk0;  // K-tiles of one plane (d_pad / BK)
  int gn;  // gallery tiles per tile-order group
  // linear epilogue: v = acc + bias; act; + resid; v * bn_scale + bn_shift
  const float* bias;
  const float* bn_scale;
  const float* bn_shift;
  const float* resid;
  int64_t ldr;
  int relu;  // activation: 0 none, 1 ReLU, 2 QuickGELU, 3 sigmoid
  // store
  void* out;
  int64_t ldo;
  float alpha, beta;
  int out_f64;
  // rank
  const float* row_hi;
  const float* row_lo;
  const float* col_hi;
  const float* col_lo;
  int* row_cnt;
  int* col_cnt;
  unsigned long long* cand;        // bucket storage (cand_layout): bucket b at cand + b * cap_b
  long long cand_cap;
  unsigned long long* cand_count;
  unsigned long long* bucket_cnt;  // per-bucket pair counters (head of the caller's buffer)
  long long cap_b;
  // rank thresholds derived in-kernel from the exact GT scores (K14): thr = dir-rounded sgt +- E(e_row,
  // err_max of the other set), the err_max reduced from the other set's per-row bounds at kernel start;
  // replaces row_hi / row_lo / col_hi / col_lo (which then only say which directions are on)
  int thr_gt;
  const double* row_sgt;
  const double* col_sgt;
  const float* q_err;  // per-row bounds of the mode's plane, [n_pad] (padding rows 0)
  const float* g_err;
  const unsigned* q_emax;  // err_max shards of the mode's plane, [EMAX_SHARDS] float bits each side
  const unsigned* g_emax;
  unsigned long long* dbg_stamps;  // kernel studies only: [tile][8] stamps, nullptr otherwise
  // K14: undecided pairs bucketed by 64 x 64 output tile (bucket (m0 >> 6) * nbn64 + (n0 >> 6)) instead of by
  // 256 gallery rows: a 1k x 1k evaluation otherwise sends every wave's slot reservation to one of 4 counters
  int tile_buckets;
  int nbn64;
  // K14: the first GT of every row / column (-1: none); the 2-stage / ring rank epilogues drop that GT pair
  // from the undecided list -- a GT item's score never exceeds its row's best GT score, so it is never counted
  const int* row_gt1;
  const int* col_gt1;
  // K14 at G64 (the ring kernel): the undecided pairs are re-scored in fp64 inside the epilogue (fixup_walk's
  // arithmetic, wave_cos64 on the raw rows) instead of being listed for a fix-up launch
  int fix_inline;
  int q_f64, g_f64;
  const void* q_raw;
  const void* g_raw;
  int64_t q_ld, g_ld, d;
  const double* q_inv;
  const double* g_inv;
  // K14 level-2 re-score (F16 rank path): the 8-bit residual planes the prep wrote beside the fp16 planes (qhi /
  // ghi) and their per-row bounds; a band pair is decided from h16 + its byte (lo8_elem) when its score clears the
  // GT score by the level-2 bound; the rest go to the level-3 list (EvalCommon::l3, re-scored in fp64 by the
  // finish), or are re-scored here when it is full.  nullptr: every pair in fp64 here
  const uint8_t* q_lo8;
  const uint8_t* g_lo8;
  const float* q_el;
  const float* g_el;
  unsigned* l3_count;
  unsigned long long* l3;
  int l3_cap;
};

// argument checks of a (q, g, mode) pair and the operand / K-loop fields of its argument block
int sim_validate_pair(const cmve_rows_t* q, const cmve_rows_t* g, int32_t mode, const char* fn);
SimArgs sim_make_args(const cmve_rows_t* q, const cmve_rows_t* g, int32_t mode);
// point the epilogue at the bucketed layout of `cand` (cand_layout) for the gallery view g
void sim_set_cand(SimArgs& a, const cmve_rows_t* g, uint64_t* cand, int64_t cand_cap, int64_t* cand_count);
// which geometry a single launch takes: the persistent G256 kernel (it reads explicit thresholds only) / the G64 ring
bool sim_uses_phased(int64_t nq_pad, int64_t ng_pad);
bool sim_uses_g64(int64_t nq_pad, int64_t ng_pad);
// the launch geometry's fields of SimArgs (the single launches fill them themselves; a batch's table is the caller's)
void sim_geo_fill(SimArgs& a, int64_t nq_pad, int64_t ng_pad, int bm, int bn);
// the rank tile of a batch of same-shaped problems
int sim_batch_geo_bm(int64_t nq_pad);
int sim_batch_geo_bn(int64_t nq_pad, int64_t ng_pad, int mode);

// the RANK epilogue over one problem, and over a device table of `count` same-shaped problems (a.nblk_m / nblk_n /
// gn of every entry from sim_geo_fill with the bm x bn passed here)
int launch_rank_gemm(const SimArgs& a, const cmve_rows_t* q, const cmve_rows_t* g, int32_t mode, hipStream_t stream);
int launch_rank_gemm_batch(const SimArgs* tab, int count, int64_t nq_pad, int64_t ng_pad, int32_t mode, int bm, int bn,
                           hipStream_t stream);

}  // namespace cmve

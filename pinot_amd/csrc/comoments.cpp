// comoments.cpp -- host-side plan of COVAR_POP / COVAR_SAMP (the reference's CovarianceAggregationFunction), alone or
// beside COUNT(*), with or without a WHERE clause and a GROUP BY.
//
// The reference keeps a CovarianceTuple (sumX, sumY, sumXY, count) per result holder and adds every doc's x, y and x y
// in doubles (CovarianceAggregationFunction.java:95-140).  Here every ordered pair of argument columns (a slot) gets
// two shifts for the call, Kx and Ky: the smallest value of each column over the queried segments, read from the
// dictionaries' first entries.  dx = x - Kx and dy = y - Ky are unsigned, so every product is non-negative, and the scan
// (scan_comoments.hip) accumulates n, sum(dx), sum(dy) and sum(dx dy).  With rx, ry the ranges of the two columns and
// N the docs of the call's segments:
//   * both columns stored as INT or LONG, rx N < 2^64 and ry N < 2^64: the integer forms -- narrow when
//     rx ry N < 2^64 (sum(dx dy) is one u64 cell that never carries), wide when rx ry N < 2^128 (a (lo, hi) pair);
//   * a FLOAT / DOUBLE column in the pair, or integer columns past those bounds: the real form, the unshifted values and
//     the three sums in double (the tuple the reference ships is the unshifted sums: a shift would buy nothing).
// dx, dy (or the doubles) come from per-segment tables over the dictIds in per-call scratch.  k_comoments_finish then
// writes the tuple of every (group, slot); COVAR_POP and COVAR_SAMP over one pair share the slot and return the same
// tuple, (x, y) and (y, x) are two slots.
//
// Stage 1, the key space, the mode rule, the statistics and the assembly of the result are the shared steps of
// scan_plan.h, with this plan's bytes per key.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "scan_plan.h"

namespace ph {

namespace {

constexpr Family kFamily{"covariance", "covariance functions"};

struct Slot {
  std::string x, y;
  int form = CFORM_NARROW;
  int64_t kx = 0, ky = 0;  // the shifts (integer forms)
  bool x_int = true, y_int = true;
};

// the shifts and the form of one slot, from the two columns' ranges over the call's segments and the call's docs; the
// bounds are checked in 128-bit arithmetic
void plan_slot(Slot& s, const std::vector<ph_segment*>& segs, double docs_queried) {
  const NumericRange x = numeric_range(kFamily, s.x, segs), y = numeric_range(kFamily, s.y, segs);
  s.x_int = x.is_int;
  s.y_int = y.is_int;
  s.form = CFORM_REAL;
  if (!x.is_int || !y.is_int) return;
  typedef unsigned __int128 u128;
  const u128 rx = (uint64_t)x.ihi - (uint64_t)x.ilo, ry = (uint64_t)y.ihi - (uint64_t)y.ilo;
  const u128 N = (uint64_t)std::max(1.0, docs_queried);
  const u128 max64 = ~(uint64_t)0, max128 = ~(u128)0;
  if (rx * N > max64 || ry * N > max64) return;  // (both factors below 2^64: the products fit 128 bits)
  s.kx = x.ilo;
  s.ky = y.ilo;
  const u128 rr = rx * ry;
  if (rr == 0 || rr <= max64 / N) s.form = CFORM_NARROW;
  else if (rr <= max128 / N) s.form = CFORM_WIDE;
}

}  // namespace

bool has_comoment_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (is_comoment(q->aggregations[k].type)) return true;
  return false;
}

void comoments_validate(const ph_query* q) {
  check_query(q);
  std::vector<std::pair<std::string, std::string>> pairs;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    refuse_plain_beside(kFamily, a);
    // (the two plans use different shifts and cell sets: DESIGN.md, "Co-moments")
    if (is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "variance function beside a covariance function");
    if (a.type != PH_AGG_COUNT && !is_comoment(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a covariance function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "covariance function of an expression argument");
    // the reference takes arguments.get(0) and get(1) (CovarianceAggregationFunction.java:57-61): a call with one
    // argument fails there
    if (!a.column || !a.column2) fail(PH_ERR_BAD_QUERY, "a covariance function needs two columns");
    const std::pair<std::string, std::string> pr(a.column, a.column2);
    if (std::find(pairs.begin(), pairs.end(), pr) == pairs.end()) pairs.push_back(pr);
  }
  if ((int)pairs.size() > kCMaxSlots)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kCMaxSlots) + " distinct column pairs under covariance functions");
  check_shape(kFamily, q);
}

ph_result* comoments_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  const auto t0 = std::chrono::steady_clock::now();
  comoments_validate(q);
  const std::vector<ph_segment*> segs = check_call(ctx, q, segs_in, nseg);

  // ---- slots (one per ordered pair of argument columns), columns, the call's docs
  const int nagg = q->num_aggregations;
  std::vector<Slot> slots;
  std::vector<int> agg_slot(nagg, -1);
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    size_t at = 0;
    while (at < slots.size() && !(slots[at].x == a.column && slots[at].y == a.column2)) ++at;
    if (at == slots.size()) {
      slots.emplace_back();
      slots.back().x = a.column;
      slots.back().y = a.column2;
    }
    agg_slot[k] = (int)at;
  }
  const int ns = (int)slots.size();
  const std::vector<std::string> group_cols = group_columns(q);
  check_columns(q, segs, group_cols);
  double docs_queried = 0.0;
  for (auto* s : segs) docs_queried += (double)s->num_docs;
  int cell_bytes = 8;  // per key: n, then 24 bytes per narrow or real slot, 32 per wide one
  std::vector<std::string> arg_cols;  // the distinct argument columns (the statistics)
  for (auto& s : slots) {
    plan_slot(s, segs, docs_queried);
    cell_bytes += s.form == CFORM_WIDE ? 32 : 24;
    for (const std::string* c : {&s.x, &s.y})
      if (std::find(arg_cols.begin(), arg_cols.end(), *c) == arg_cols.end()) arg_cols.push_back(*c);
  }

  // ---- the WHERE clause's class per segment, the key space, the mode
  std::vector<int32_t> cls((size_t)nseg);
  for (int i = 0; i < nseg; ++i) cls[i] = where_class(q, segs[i]);
  const KeySpace ks = key_space(kFamily, group_cols, segs);
  const int64_t G = ks.G;
  refuse_group_limit(kFamily, q, ks, segs, cls);
  // tables: n, four accumulator cells and the 32-byte tuple per slot (so G stays far below 2^32: the scan's keys are
  // uint32)
  const int mode = choose_mode(ctx, kFamily, ks, (double)G * (8.0 + 64.0 * ns), (double)G * cell_bytes);

  auto res = new_result(ctx, segs);
  ph_exec_stats& stats = res->stats;
  double dev_ms = 0.0;

  LaneGuard lane(ctx);
  const hipStream_t st = lane.stream();
  // host sources of the stream's H2D copies: declared before `scratch`, whose destructor drains the stream, so they
  // outlive every copy also when the call unwinds by a throw
  std::vector<CSegment> msegs;
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<std::vector<uint64_t>> d_of_keep;
  std::vector<CSlot> launch_slots;
  std::vector<unsigned long long> host_tables;  // (and the target of the result's D2H copies)
  Scratch scratch(ctx, st);

  // ---- stage 1: the WHERE clause's doc bitmap per segment where it neither matches all nor is empty
  std::vector<WhereBitmap> bitmap((size_t)nseg);
  for (int i = 0; i < nseg; ++i)
    if (cls[i] != FP_EMPTY && cls[i] != FP_ALL) bitmap[i] = where_bitmap(ctx, q, q->filter_root, segs[i], scratch, dev_ms);
  check_interrupt(q);

  // ---- stage 2: device segments (with each slot's two tables over the dictIds), chunks, tables
  int max_bits = 1;
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    CSegment d{};
    d.num_docs = segs[i]->num_docs;
    d.mask = bitmap[i].words;
    group_streams(ks, segs[i], d.gfwd, d.gbits, d.gremap, scratch, remap_keep, st);
    for (size_t g = 0; g < group_cols.size(); ++g) max_bits = std::max(max_bits, (int)d.gbits[g]);
    for (int v = 0; v < ns; ++v) {
      const Slot& s = slots[(size_t)v];
      // dictId -> x - Kx as a u64 (integer forms), or the bits of (double) x
      auto table_of = [&](const std::string& col, bool is_int, int64_t shift, const uint32_t*& fwd, int32_t& bits) {
        const Column& c = *segs[i]->columns.at(col);
        if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "covariance column " + col + " has no forward index");
        std::vector<uint64_t> tab((size_t)std::max(1, c.cardinality), 0);
        for (int32_t id = 0; id < c.cardinality; ++id) {
          if (s.form != CFORM_REAL) {
            tab[(size_t)id] = (uint64_t)c.dict.ints[(size_t)id] - (uint64_t)shift;
          } else {
            const double x = is_int ? (double)c.dict.ints[(size_t)id] : c.dict.reals[(size_t)id];
            memcpy(&tab[(size_t)id], &x, 8);
          }
        }
        unsigned long long* dt = scratch.alloc<unsigned long long>(tab.size());
        d_of_keep.push_back(std::move(tab));
        PH_HIP_CHECK(hipMemcpyAsync(dt, d_of_keep.back().data(), 8 * d_of_keep.back().size(), hipMemcpyHostToDevice, st));
        fwd = c.d_fwd.as<uint32_t>();
        bits = c.bits;
        max_bits = std::max(max_bits, (int)c.bits);
        return dt;
      };
      d.pair[v].x_of = table_of(s.x, s.x_int, s.kx, d.pair[v].xfwd, d.pair[v].xbits);
      d.pair[v].y_of = table_of(s.y, s.y_int, s.ky, d.pair[v].yfwd, d.pair[v].ybits);
    }
    append_chunks(chunks, (int32_t)msegs.size(), d.num_docs);
    msegs.push_back(d);
  }
  // u64 cells: [segments] matched docs | n[G] | per slot S1x[G], S1y[G], Sxy lo[G], Sxy hi[G] | per slot the CTuple[G] of
  // the finish
  const size_t nms = msegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nms);
  const size_t acc_cells = (size_t)G * (1 + 4 * (size_t)ns);
  const size_t out_off = cnt_cells + acc_cells;
  const size_t cells = out_off + 4 * (size_t)G * (size_t)ns;
  host_tables.assign(cells, 0ull);  // (a CTuple of zero bits is (0.0, 0.0, 0.0, 0))
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(cells);
    CSegment* d_segs = scratch.alloc<CSegment>(nms);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    CSlot* d_slots = scratch.alloc<CSlot>((size_t)ns);
    unsigned long long* n_tab = tables + cnt_cells;
    auto cell = [&](int slot, int which) { return n_tab + (size_t)G * (1 + 4 * (size_t)slot + (size_t)which); };
    // the launches' slots, grouped by form
    int form_begin[4] = {0, 0, 0, 0};
    for (int form = CFORM_NARROW; form <= CFORM_REAL; ++form) {
      for (int v = 0; v < ns; ++v)
        if (slots[(size_t)v].form == form) launch_slots.push_back(CSlot{v, cell(v, 0), cell(v, 1), cell(v, 2), cell(v, 3)});
      form_begin[form + 1] = (int)launch_slots.size();
    }
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, msegs.data(), sizeof(CSegment) * nms, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_slots, launch_slots.data(), sizeof(CSlot) * launch_slots.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * out_off, st));
    CFinishParams fin{};
    fin.num_groups = G;
    fin.num_slots = ns;
    fin.n = n_tab;
    for (int v = 0; v < ns; ++v) {
      fin.form[v] = slots[(size_t)v].form;
      fin.kx[v] = slots[(size_t)v].kx;
      fin.ky[v] = slots[(size_t)v].ky;
      fin.s1x[v] = cell(v, 0);
      fin.s1y[v] = cell(v, 1);
      fin.sxy[v] = cell(v, 2);
      fin.sxyhi[v] = cell(v, 3);
      fin.out[v] = reinterpret_cast<CTuple*>(tables + out_off + 4 * (size_t)G * (size_t)v);
    }
    const int grid = scan_grid(ctx, mode, chunks.size());
    // one launch per form among the slots; the first one counts the docs (n and the segments' matched docs)
    bool counted = false;
    for (int form = CFORM_NARROW; form <= CFORM_REAL; ++form) {
      CParams cp{};
      cp.segs = d_segs;
      cp.chunks = d_chunks;
      cp.slots = d_slots + form_begin[form];
      cp.num_slots = form_begin[form + 1] - form_begin[form];
      if (!cp.num_slots) continue;
      cp.chunk_end = (int32_t)chunks.size();
      cp.num_group_cols = (int32_t)group_cols.size();
      for (int g = 0; g < kMaxGroupCols; ++g) cp.group_stride[g] = (uint32_t)ks.stride[g];
      cp.num_groups = G;
      if (!counted) {
        cp.n = n_tab;
        cp.seg_count = tables;
        counted = true;
      }
      launch_scan_comoments(cp, mode, form, max_bits, grid, st);
    }
    launch_comoments_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * (cnt_cells + (size_t)G), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + out_off, tables + out_off, 8 * (cells - out_off),
                                hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_COMOMENTS;

  // ---- statistics (docs x the group-by and distinct argument columns); result rows: a group is a row when it holds a
  // doc; an aggregation-only query has one row, (0.0, 0.0, 0.0, 0) where nothing matched
  // (CovarianceAggregationFunction.extractAggregationResult :155-162)
  add_scan_stats(stats, host_tables.data(), nms, (int64_t)(group_cols.size() + arg_cols.size()), bitmap);
  emit_rows(res.get(), q, ks, host_tables.data() + cnt_cells, agg_slot,
            reinterpret_cast<const uint8_t*>(host_tables.data() + out_off), sizeof(CTuple));
  finish_result(res.get(), mode, dev_ms, t0);
  return res.release();
}

}  // namespace ph

// moments4.cpp -- host-side plan of SKEWNESS / KURTOSIS (the reference's FourthMomentAggregationFunction over
// PinotFourthMoment), alone or beside COUNT(*), with or without a WHERE clause and a GROUP BY.
//
// The reference keeps a PinotFourthMoment (n, m1, m2, m3, m4) per result holder and folds every doc in with
// commons-math's one-pass update.  Here every argument column (a slot) gets a shift K for the call, taken from the first
// and last dictionary entries of the column in every queried segment, and the scan (scan_moments4.hip) accumulates n
// and the power sums S1..S4 of d = value - K:
//   * a column stored as INT or LONG whose range r = hi - lo over the call is below 2^32, in a call of at most 2^32
//     docs: K = lo, so 0 <= d <= r, and every power is split into 32-bit limbs with a 64-bit cell each -- M4_L8 when
//     r < 2^8 (4 cells), M4_L16 when r < 2^16 (6 cells), M4_L32 otherwise (10 cells);
//   * FLOAT / DOUBLE columns and integer columns past those bounds: M4_REAL, K the midpoint as a double and the four
//     sums in double.
// d comes from a per-segment table d_of[dictId] in per-call scratch, so the scan does one lookup per doc.
// k_moments4_finish then writes the tuple of every (group, slot); the two functions over one column share the slot and
// return the same tuple.
//
// Stage 1, the key space, the mode rule, the statistics and the assembly of the result are the shared steps of
// scan_plan.h, with this plan's bytes per key.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "scan_plan.h"

namespace ph {

namespace {

constexpr Family kFamily{"fourth-moment", "fourth-moment functions"};

struct Slot {
  std::string col;
  int layout = M4_L8;
  int64_t shift = 0;  // K: an int64, or a double's bits (M4_REAL)
  bool is_int = true;
};

// the shift and the layout of one slot, from the column's range over the call's segments and the call's docs
void plan_slot(Slot& s, const std::vector<ph_segment*>& segs, double docs_queried) {
  const NumericRange nr = numeric_range(kFamily, s.col, segs);
  s.is_int = nr.is_int;
  if (s.is_int) {
    const uint64_t r = (uint64_t)nr.ihi - (uint64_t)nr.ilo;
    // a limb cell holds docs x (2^32 - 1) at most: exact to 2^32 docs
    if (r < (1ull << 32) && docs_queried <= 4294967296.0) {
      s.layout = r < (1ull << 8) ? M4_L8 : (r < (1ull << 16) ? M4_L16 : M4_L32);
      s.shift = nr.ilo;
      return;
    }
  }
  const double kd = 0.5 * nr.lo + 0.5 * nr.hi;
  s.layout = M4_REAL;
  memcpy(&s.shift, &kd, 8);
}

}  // namespace

bool has_moment4_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (is_moment4(q->aggregations[k].type)) return true;
  return false;
}

void moments4_validate(const ph_query* q) {
  check_query(q);
  std::vector<std::string> cols;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    refuse_plain_beside(kFamily, a);
    if (is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "variance function beside a fourth-moment function");
    if (is_comoment(a.type)) fail(PH_ERR_UNSUPPORTED, "covariance function beside a fourth-moment function");
    if (a.type != PH_AGG_COUNT && !is_moment4(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a fourth-moment function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "fourth-moment function of a 2-operand expression");
    if (!a.column) fail(PH_ERR_BAD_QUERY, "aggregation needs a column");
    if (std::find(cols.begin(), cols.end(), std::string(a.column)) == cols.end()) cols.push_back(a.column);
  }
  if ((int)cols.size() > kMMaxSlots)
    fail(PH_ERR_UNSUPPORTED,
         "more than " + std::to_string(kMMaxSlots) + " distinct columns under fourth-moment functions");
  check_shape(kFamily, q);
}

ph_result* moments4_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  const auto t0 = std::chrono::steady_clock::now();
  moments4_validate(q);
  const std::vector<ph_segment*> segs = check_call(ctx, q, segs_in, nseg);

  // ---- slots (one per argument column), columns, the call's docs
  const int nagg = q->num_aggregations;
  std::vector<Slot> slots;
  std::vector<int> agg_slot(nagg, -1);
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    size_t at = 0;
    while (at < slots.size() && slots[at].col != a.column) ++at;
    if (at == slots.size()) {
      slots.emplace_back();
      slots.back().col = a.column;
    }
    agg_slot[k] = (int)at;
  }
  const int ns = (int)slots.size();
  const std::vector<std::string> group_cols = group_columns(q);
  check_columns(q, segs, group_cols);
  double docs_queried = 0.0;
  for (auto* s : segs) docs_queried += (double)s->num_docs;
  // per key: n, then 8 bytes per cell of every slot's layout; slot v's cells start at cell_off[v]
  size_t acc_per_key = 1;
  std::vector<size_t> cell_off((size_t)ns, 0);
  for (int v = 0; v < ns; ++v) {
    plan_slot(slots[(size_t)v], segs, docs_queried);
    cell_off[(size_t)v] = acc_per_key;
    acc_per_key += (size_t)m4_cells(slots[(size_t)v].layout);
  }
  constexpr size_t kTupleCells = sizeof(M4Tuple) / 8;

  // ---- the WHERE clause's class per segment, the key space, the mode
  std::vector<int32_t> cls((size_t)nseg);
  for (int i = 0; i < nseg; ++i) cls[i] = where_class(q, segs[i]);
  const KeySpace ks = key_space(kFamily, group_cols, segs);
  const int64_t G = ks.G;
  refuse_group_limit(kFamily, q, ks, segs, cls);
  // tables: n, the slots' cells and the 40-byte tuple per slot
  const int mode = choose_mode(ctx, kFamily, ks, (double)G * 8.0 * (double)(acc_per_key + kTupleCells * (size_t)ns),
                               (double)G * 8.0 * (double)acc_per_key);

  auto res = new_result(ctx, segs);
  ph_exec_stats& stats = res->stats;
  double dev_ms = 0.0;

  LaneGuard lane(ctx);
  const hipStream_t st = lane.stream();
  // host sources of the stream's H2D copies: declared before `scratch`, whose destructor drains the stream, so they
  // outlive every copy also when the call unwinds by a throw
  std::vector<MSegment> msegs;
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<std::vector<int64_t>> d_of_keep;
  std::vector<unsigned long long> host_tables;  // (and the target of the result's D2H copies)
  Scratch scratch(ctx, st);

  // ---- stage 1: the WHERE clause's doc bitmap per segment where it neither matches all nor is empty
  std::vector<WhereBitmap> bitmap((size_t)nseg);
  for (int i = 0; i < nseg; ++i)
    if (cls[i] != FP_EMPTY && cls[i] != FP_ALL) bitmap[i] = where_bitmap(ctx, q, q->filter_root, segs[i], scratch, dev_ms);
  check_interrupt(q);

  // ---- stage 2: device segments (with each slot's d_of table), chunks, tables
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    MSegment d{};
    d.num_docs = segs[i]->num_docs;
    d.mask = bitmap[i].words;
    group_streams(ks, segs[i], d.gfwd, d.gbits, d.gremap, scratch, remap_keep, st);
    for (int v = 0; v < ns; ++v) {
      const Slot& s = slots[(size_t)v];
      const Column& c = *segs[i]->columns.at(s.col);
      if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "fourth-moment column " + s.col + " has no forward index");
      std::vector<int64_t> tab((size_t)std::max(1, c.cardinality), 0);
      double kd;
      memcpy(&kd, &s.shift, 8);
      for (int32_t id = 0; id < c.cardinality; ++id) {
        if (s.layout != M4_REAL) {
          tab[(size_t)id] = (int64_t)((uint64_t)c.dict.ints[(size_t)id] - (uint64_t)s.shift);  // 0 <= d < 2^32
        } else {
          const double x = (s.is_int ? (double)c.dict.ints[(size_t)id] : c.dict.reals[(size_t)id]) - kd;
          memcpy(&tab[(size_t)id], &x, 8);
        }
      }
      long long* dt = scratch.alloc<long long>(tab.size());
      d_of_keep.push_back(std::move(tab));
      PH_HIP_CHECK(hipMemcpyAsync(dt, d_of_keep.back().data(), 8 * d_of_keep.back().size(), hipMemcpyHostToDevice, st));
      d.vfwd[v] = c.d_fwd.as<uint32_t>();
      d.d_of[v] = dt;
      d.vbits[v] = c.bits;
    }
    append_chunks(chunks, (int32_t)msegs.size(), d.num_docs);
    msegs.push_back(d);
  }
  // u64 cells: [segments] matched docs | n[G] | per slot its layout's cells, [G] each | per slot the M4Tuple[G] of the
  // finish
  const size_t nms = msegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nms);
  const size_t out_off = cnt_cells + (size_t)G * acc_per_key;
  const size_t cells = out_off + kTupleCells * (size_t)G * (size_t)ns;
  host_tables.assign(cells, 0ull);
  {  // no launch (no segment left to scan): every tuple is the empty one, (0, NaN, NaN, NaN, NaN)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const M4Tuple empty{0, nan, nan, nan, nan};
    for (size_t i = 0; i < (size_t)G * (size_t)ns; ++i) memcpy(&host_tables[out_off + kTupleCells * i], &empty, sizeof(empty));
  }
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(cells);
    MSegment* d_segs = scratch.alloc<MSegment>(nms);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, msegs.data(), sizeof(MSegment) * nms, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * out_off, st));
    unsigned long long* n_tab = tables + cnt_cells;
    M4FinishParams fin{};
    fin.num_groups = G;
    fin.num_slots = ns;
    fin.n = n_tab;
    for (int v = 0; v < ns; ++v) {
      fin.layout[v] = slots[(size_t)v].layout;
      fin.shift[v] = slots[(size_t)v].shift;
      fin.cells[v] = n_tab + (size_t)G * cell_off[(size_t)v];
      fin.out[v] = reinterpret_cast<M4Tuple*>(tables + out_off + kTupleCells * (size_t)G * (size_t)v);
    }
    const int grid = scan_grid(ctx, mode, chunks.size());
    // one launch per layout among the slots; the first one counts the docs (n and the segments' matched docs)
    bool counted = false;
    for (int layout = M4_L8; layout <= M4_REAL; ++layout) {
      M4Params mp{};
      mp.segs = d_segs;
      mp.chunks = d_chunks;
      mp.chunk_end = (int32_t)chunks.size();
      mp.num_group_cols = (int32_t)group_cols.size();
      std::copy(ks.stride, ks.stride + kMaxGroupCols, mp.group_stride);
      mp.num_groups = G;
      for (int v = 0; v < ns; ++v) {
        if (slots[(size_t)v].layout != layout) continue;
        const int at = mp.num_slots++;
        mp.slot_col[at] = v;
        mp.cells[at] = n_tab + (size_t)G * cell_off[(size_t)v];
      }
      if (!mp.num_slots) continue;
      if (!counted) {
        mp.n = n_tab;
        mp.seg_count = tables;
        counted = true;
      }
      launch_scan_moments4(mp, mode, layout, grid, st);
    }
    launch_moments4_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * (cnt_cells + (size_t)G), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + out_off, tables + out_off, 8 * (cells - out_off),
                                hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_MOMENTS4;

  // ---- statistics (docs x the group-by and argument columns); result rows: a group is a row when it holds a doc; an
  // aggregation-only query has one row, the empty tuple where nothing matched
  add_scan_stats(stats, host_tables.data(), nms, (int64_t)group_cols.size() + ns, bitmap);
  emit_rows(res.get(), q, ks, host_tables.data() + cnt_cells, agg_slot,
            reinterpret_cast<const uint8_t*>(host_tables.data() + out_off), sizeof(M4Tuple));
  finish_result(res.get(), mode, dev_ms, t0);
  return res.release();
}

}  // namespace ph

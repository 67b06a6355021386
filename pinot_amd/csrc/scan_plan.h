// scan_plan.h -- the host-side steps that the bitmap-then-scan plans share: filtered aggregations (filtered.cpp), the
// variance family (moments.cpp), COVAR (comoments.cpp), SKEWNESS / KURTOSIS (moments4.cpp), HISTOGRAM (bins.cpp) and
// FIRSTWITHTIME / LASTWITHTIME (withtime.cpp).  Each of those planners
// reads top to bottom as a list of steps; the steps that are the same in all of them live here (scan_plan.cpp), once:
// the call checks, the range of an argument column, the WHERE clause's class and doc bitmap per segment, the dense key
// space with its refusals and the mode rule, a segment's group-by streams and chunks, and the assembly of the result.
// Host only: no kernel and no struct a kernel reads is declared here.
#pragma once

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "ph_internal.h"

namespace ph {

inline bool is_moment(int32_t t) { return t >= PH_AGG_VARPOP && t <= PH_AGG_STDDEVSAMP; }
inline bool is_comoment(int32_t t) { return t == PH_AGG_COVARPOP || t == PH_AGG_COVARSAMP; }
inline bool is_moment4(int32_t t) { return t == PH_AGG_SKEWNESS || t == PH_AGG_KURTOSIS; }

// how a plan's refusals name it: {"variance", "variance functions"}, {"filtered", "filtered aggregations"}
struct Family {
  const char* word;
  const char* plural;
};

// ---- *_validate
void check_query(const ph_query* q);  // a query with a well-formed aggregation list
// SUM / MIN / MAX / DISTINCTCOUNTHLL / DISTINCTCOUNT / PERCENTILE: "<FN> beside a <word> function"
void refuse_plain_beside(const Family& f, const ph_aggregation& a);
// at most kMaxAggs aggregations and kMaxGroupCols group-by columns, no segment group trim
void check_shape(const Family& f, const ph_query* q);

// ---- the call
std::vector<ph_segment*> check_call(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg);
void check_interrupt(const ph_query* q);  // (check_call makes both checks)
void check_deadline(const ph_query* q);
std::vector<std::string> group_columns(const ph_query* q);
const Column& column_in(const ph_segment* seg, const std::string& col);  // refuses a column the segment lacks
// every group-by and predicate column is in every segment
void check_columns(const ph_query* q, const std::vector<ph_segment*>& segs, const std::vector<std::string>& group_cols);

// one numeric argument column over the call's segments, from its dictionaries' first and last entries: lo and hi are
// (double) ilo and ihi for a column stored as INT or LONG.  Refuses STRING, sketch and mixed integer/real columns
struct NumericRange {
  bool is_int = true, any = false;  // any: some segment's dictionary has an entry
  int64_t ilo = 0, ihi = 0;
  double lo = 0.0, hi = 0.0;
};
NumericRange numeric_range(const Family& f, const std::string& col, const std::vector<ph_segment*>& segs);

// how the WHERE clause plans on a segment (FilterPlanNode.run's isResultEmpty / isResultMatchingAll): its
// filter_plan_class, or without one FP_ALL (FP_EMPTY for a segment of 0 docs)
int32_t where_class(const ph_query* q, ph_segment* seg);

// stage 1: `root` planned as a WHERE clause over one segment (query_execute_impl's COUNT(*) + doc bitmap form, never
// from a star-tree).  The bitmap is in `scratch`; the call has drained its stream when it returns
struct WhereBitmap {
  unsigned long long* words = nullptr;
  int64_t docs = 0, entries = 0;  // matched docs; the filter's ordinary numEntriesScannedInFilter
};
WhereBitmap where_bitmap(Context* ctx, const ph_query* q, int32_t root, ph_segment* seg, Scratch& scratch, double& dev_ms);

// the dense key space of a call: union-dictionary ids, G = prod(sizes) (1 without a group-by), key = sum(id[g] stride[g])
struct KeySpace {
  std::vector<std::string> group_cols;
  std::vector<std::shared_ptr<GlobalDict>> gdicts;
  int64_t G = 1;
  int64_t stride[kMaxGroupCols] = {};
  int64_t size(size_t g) const { return std::max<int64_t>(1, gdicts[g]->dict.size); }
};
KeySpace key_space(const Family& f, const std::vector<std::string>& group_cols, const std::vector<ph_segment*>& segs);
// refuses a call in which a segment that `cls` does not leave empty could reach numGroupsLimit
void refuse_group_limit(const Family& f, const ph_query* q, const KeySpace& ks, const std::vector<ph_segment*>& segs,
                        const std::vector<int32_t>& cls);
// refuses tables of `table_bytes` beyond the dense budget; then MODE_AGG without a group-by, MODE_GROUP_LDS when
// `lds_bytes` (G x the bytes a block keeps per key) fits OPT_LDS_TABLE_MAX, MODE_GROUP_GLOBAL otherwise
int choose_mode(Context* ctx, const Family& f, const KeySpace& ks, double table_bytes, double lds_bytes);
int scan_grid(const Context* ctx, int mode, size_t num_chunks);

std::unique_ptr<ph_result> new_result(Context* ctx, const std::vector<ph_segment*>& segs);

// stage 2, one segment: its group-by streams into gfwd / gbits / gremap[0 .. group columns) of an FSegment, MSegment or
// CSegment.  A column whose dictionary is not the union dictionary gets a remap table in `scratch`, copied on `st` from
// a vector appended to `remap_keep`: the caller declares `remap_keep` before `scratch`, whose destructor drains the
// stream, so that the source outlives the copy also when the call unwinds by a throw
void group_streams(const KeySpace& ks, const ph_segment* seg, const uint32_t** gfwd, int32_t* gbits, const int32_t** gremap,
                   Scratch& scratch, std::vector<std::vector<int32_t>>& remap_keep, hipStream_t st);
// the kChunkWords chunks of device segment `seg_index`
void append_chunks(std::vector<Chunk>& chunks, int32_t seg_index, int32_t num_docs);

// ---- the result
// matched docs per device segment (`seg_count`), the WHERE clause's ordinary statistic, docs x projected columns
void add_scan_stats(ph_exec_stats& stats, const unsigned long long* seg_count, size_t num_device_segs, int64_t projected,
                    const std::vector<WhereBitmap>& bitmaps);
// the key columns of the rows (dense keys)
void emit_keys(ph_result* res, const KeySpace& ks, const std::vector<int64_t>& rows);
// the rows of a plan whose aggregations are COUNT(*) (n_host[key]) or a fixed-width tuple of a slot
// (tuples + tuple_bytes (G slot + key)): the keys with n != 0, or one row for an aggregation-only query
void emit_rows(ph_result* res, const ph_query* q, const KeySpace& ks, const unsigned long long* n_host,
               const std::vector<int>& agg_slot, const uint8_t* tuples, size_t tuple_bytes);
// the same with a width per slot (bins.cpp): slot v's tuples, slot_bytes[v] each, [G] of them, follow slot v - 1's
void emit_rows(ph_result* res, const ph_query* q, const KeySpace& ks, const unsigned long long* n_host,
               const std::vector<int>& agg_slot, const uint8_t* tuples, const std::vector<size_t>& slot_bytes);
// plan_mode, num_devices, device_ms, and host_ms = the time since t0 that is not device time
void finish_result(ph_result* res, int mode, double dev_ms, std::chrono::steady_clock::time_point t0);

}  // namespace ph

// rtow_sorted_list.h — the per-lane sorted list of the ordered queries: eight (key, walk id) pairs in registers, ascending
// by (key, insertion index).  Included inside namespace rtow { namespace { ... } } by rtow_first_hits.h (key: the ray
// parameter t) and rtow_nearest.h (key: the distance).
//
// Insertion is a fully unrolled compare-and-shift over eight named slots.  The insertion index (`map[id]`) is read only
// to break an exact tie in the key.  A primitive tested again after it was evicted is rejected by the ordering itself.
// The list always sorts 8: slots at and beyond the caller's cut may hold entries past it; they are not reported.

// Eight named slots, not arrays: the compiler folds a chain of selects over array elements into one dynamically indexed
// load, which sends the whole list to scratch; named members are registers from the first pass on.
#define RTOW_SL_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
struct SortedList8 {
  double t0, t1, t2, t3, t4, t5, t6, t7;  // keys, ascending by (key, map[id]); an empty slot holds `fill` (no kept key is above it)
  int i0, i1, i2, i3, i4, i5, i6, i7;     // walk ids; -1 = empty slot (empty slots are a suffix)
};
// `fill`: the query's own bound (tmax in the walk's ray parameter, max_dist)
__device__ __forceinline__ void list_clear(SortedList8 &L, double fill) {
#define RTOW_SL_X(j) L.t##j = fill, L.i##j = -1;
  RTOW_SL_SLOTS(RTOW_SL_X)
#undef RTOW_SL_X
}
// The culling bound: the key of slot n - 1 — `fill` while fewer than n entries are kept (an empty slot holds it, so the
// walk keeps no copy of it), then the key of the last entry that will be reported.
__device__ __forceinline__ double list_bound(const SortedList8 &L, int n) {
  double b = L.t7;
#define RTOW_SL_X(j) if (n == j + 1) b = L.t##j;
  RTOW_SL_SLOTS(RTOW_SL_X)
#undef RTOW_SL_X
  return b;
}
// Entry j of the list (wave-uniform j).  (The empty asm keeps the selects a chain: left alone, the compiler parks the
// eight keys in scratch and loads slot j from there.)
__device__ __forceinline__ void list_entry(const SortedList8 &L, int j, double &t, int &id) {
  t = L.t7, id = L.i7;
#define RTOW_SL_X(k)                  \
  if (j == k) t = L.t##k, id = L.i##k; \
  asm volatile("" : "+v"(t), "+v"(id));
  RTOW_SL_SLOTS(RTOW_SL_X)
#undef RTOW_SL_X
}
// Inserts (t, id) in (t, map[id]) order by compare-and-shift over the eight slots; the entry pushed out of slot 7, or
// the candidate itself, is dropped.
// DEDUP: drop a candidate whose primitive is already kept (a walk that can meet a primitive twice).
template <bool DEDUP>
__device__ __forceinline__ void list_insert(SortedList8 &L, double t, int id, const int32_t *map) {
  if constexpr (DEDUP) {
    bool dup = false;
#define RTOW_SL_X(j) dup = dup || L.i##j == id;
    RTOW_SL_SLOTS(RTOW_SL_X)
#undef RTOW_SL_X
    if (dup) return;
  }
  // b<j>: entry j stays in front of the candidate (a prefix of the list, which is sorted); an exact tie in the key is
  // decided by the insertion index
#define RTOW_SL_X(j)                                              \
  bool b##j = L.t##j < t;                                         \
  if (L.t##j == t && L.i##j >= 0) b##j = map[L.i##j] < map[id];
  RTOW_SL_SLOTS(RTOW_SL_X)
#undef RTOW_SL_X
#define RTOW_SL_SHIFT(j, jm)            \
  if (!b##j) {                          \
    L.t##j = b##jm ? t : L.t##jm;       \
    L.i##j = b##jm ? id : L.i##jm;      \
  }
  RTOW_SL_SHIFT(7, 6)
  RTOW_SL_SHIFT(6, 5)
  RTOW_SL_SHIFT(5, 4)
  RTOW_SL_SHIFT(4, 3)
  RTOW_SL_SHIFT(3, 2)
  RTOW_SL_SHIFT(2, 1)
  RTOW_SL_SHIFT(1, 0)
#undef RTOW_SL_SHIFT
  if (!b0) {
    L.t0 = t;
    L.i0 = id;
  }
}

// mh_parts.hpp -- one kernel template, one source, several objects.  A template with more instantiations than one compile should
// carry still keeps its whole table in one k_*.hip, which is compiled once per PART with -DFMH_PART=<name> into build/k_<name>.o
// (fmcmc_amd/build.py reads the names off the FMH_PARTS line, so they are written there only).  The source defines, in this order,
//   #define FMH_PARTS(X) X(lat1a) X(lat1b) ...             its parts, on one line
//   #define FMH_LOOKUPS_lat1a 1                            the first part: its object also holds the public look-ups (mh_kernels.hpp)
//   #define FMH_KERNEL(KIND, FAM, P) mh_sweep_lat<...>     the instantiation a key stands for
//   #define FMH_TABLE(R) R(lat1a, 1, LINREG, 0) ...        a row = the part that compiles the instantiation, then its key
// and includes this header, which makes of them
//   k_part_<name>(key, n)   one per part, defined by the compile of that part: the key among the rows of its own part.  The rows sit
//                           in a template over the part, so that `if constexpr` drops the others uninstantiated;
//   find_kernel(ints...)    (first part) asks the parts in turn; nullptr: no row has the key.
// A row's key and its template arguments are the same tokens; a row that names no part of FMH_PARTS does not compile.
#pragma once
#ifndef FMH_PART
#error "a source with FMH_PARTS is compiled once per part, with -DFMH_PART=<part>"
#endif
#define FMH_CAT_(a, b) a##b
#define FMH_CAT(a, b) FMH_CAT_(a, b)
#define FMH_HAS_LOOKUPS FMH_CAT(FMH_LOOKUPS_, FMH_PART)

// rows that differ in their last key alone (p, mostly): R(args..., p) for a range of p
#define FMH_P1_3(R, ...) R(__VA_ARGS__, 1) R(__VA_ARGS__, 2) R(__VA_ARGS__, 3)
#define FMH_P4_7(R, ...) R(__VA_ARGS__, 4) R(__VA_ARGS__, 5) R(__VA_ARGS__, 6) R(__VA_ARGS__, 7)
#define FMH_P8_11(R, ...) R(__VA_ARGS__, 8) R(__VA_ARGS__, 9) R(__VA_ARGS__, 10) R(__VA_ARGS__, 11)
#define FMH_P12_14(R, ...) R(__VA_ARGS__, 12) R(__VA_ARGS__, 13) R(__VA_ARGS__, 14)
#define FMH_P1_7(R, ...) FMH_P1_3(R, __VA_ARGS__) FMH_P4_7(R, __VA_ARGS__)
#define FMH_P0_7(R, ...) R(__VA_ARGS__, 0) FMH_P1_7(R, __VA_ARGS__)
#define FMH_P8_14(R, ...) FMH_P8_11(R, __VA_ARGS__) FMH_P12_14(R, __VA_ARGS__)
#define FMH_P8_15(R, ...) FMH_P8_14(R, __VA_ARGS__) R(__VA_ARGS__, 15)

namespace fmh {
namespace part {
#define FMH_X(name) name,
enum { FMH_PARTS(FMH_X) };
#undef FMH_X
constexpr int self = FMH_PART;
}  // namespace part
#define FMH_X(name) FMH_HIDDEN const void* k_part_##name(const int* key, int n);
FMH_PARTS(FMH_X)
#undef FMH_X

namespace {
template <int... V>
bool key_is(const int* key, int n) {
  int i = 0;
  return n == (int)sizeof...(V) && ((key[i++] == V) && ...);
}
template <int PT>
const void* find_in_part(const int* key, int n) {
#define FMH_ROW(PART, ...) \
  if constexpr (PT == part::PART) if (key_is<__VA_ARGS__>(key, n)) return (const void*)FMH_KERNEL(__VA_ARGS__);
  FMH_TABLE(FMH_ROW)
#undef FMH_ROW
  return nullptr;
}
}  // namespace
const void* FMH_CAT(k_part_, FMH_PART)(const int* key, int n) { return find_in_part<part::self>(key, n); }

#if FMH_HAS_LOOKUPS
static_assert(part::self == 0, "the public look-ups belong to the first part of FMH_PARTS");
namespace {
template <class... T>
const void* find_kernel(T... k) {
  const int key[] = {(int)k...};
  const void* h = nullptr;
#define FMH_X(name) if (!h) h = k_part_##name(key, (int)sizeof...(T));
  FMH_PARTS(FMH_X)
#undef FMH_X
  return h;
}
}  // namespace
#endif
}  // namespace fmh

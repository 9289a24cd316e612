// mh_sigtree.hpp -- look-ahead tree for the sigma-only half of the Gaussian closed form (mh_sweep_mfma's owner waves).
// The sigma a proposal carries is th0 + (mu + scale z) of the state the decisions before it left, and the variates z of all
// coming steps already lie in the fed stream: the proposal sigma of step v + d is one of 2^d values fixed by the accept / reject
// pattern of the d decisions before it.  1 + 2 + .. + 32 = 63 candidates cover six steps, one per lane: ONE lane-parallel pass of
// the code an owner used to run every step (where it computed one double per wave) prepares n (log sigma + c), sigma^2, 1 / sigma^2
// and the two flags for six steps, and a step only looks up the node its realised decisions led to.  Each lane runs the source
// expressions of the owner's propose() and of the closed form on the same doubles: the bits are those of the per-step form.
#pragma once

namespace {

constexpr int ST_DEPTH = 6;                        // steps one pass covers
constexpr int ST_NODES = (1 << ST_DEPTH) - 1;      // 63 candidates, node == lane; an index >= ST_NODES asks for a rebuild
constexpr int ST_LOOK = ST_DEPTH - 1;              // stream rows a pass reads: the variates of the decisions inside the tree
constexpr int ST_ZLANE = 32;                       // lanes ST_ZLANE .. ST_ZLANE + ST_LOOK - 1 of an owner carry sigma's variate of the rows ahead
constexpr int ST_ENTRY = 4;                        // doubles per node: n t1, sigma^2, 1 / sigma^2, flags (bit 0 sg_fast, bit 1 ok_fast)
constexpr int ST_TAB = 64 * ST_ENTRY;              // doubles per owner (lane 63 writes a node nobody reads)
constexpr int ST_STALE = ST_NODES / 2;             // what the rare branch leaves: both children ask for a rebuild

constexpr int st_depth(int node) { int d = 0; while ((2 << d) - 1 <= node) d++; return d; }   // floor(log2(node + 1))
constexpr int st_path(int node) { return node + 1 - (1 << st_depth(node)); }                  // decisions, the first one in the top bit
constexpr int st_child(int node, int accept) { return 2 * node + 1 + accept; }
constexpr bool st_consistent() {
  for (int i = 0; i < ST_NODES; i++) {
    if (st_depth(i) >= ST_DEPTH || st_path(i) >> st_depth(i)) return false;
    for (int a = 0; a < 2; a++) {
      const int c = st_child(i, a);
      if (st_depth(c) != st_depth(i) + 1 || st_path(c) != 2 * st_path(i) + a) return false;   // distinct (depth, path): distinct nodes
      if ((st_depth(i) == ST_DEPTH - 1) != (c >= ST_NODES)) return false;                     // the sixth look-up is the last
    }
  }
  return st_depth(0) == 0 && st_child(ST_STALE, 0) >= ST_NODES && ST_ZLANE + ST_LOOK <= 64;
}
static_assert(st_consistent(), "tree indices");

// One pass of an owner wave.  th0 / th1: the owner's lanes (sigma in lane k - 1; th1 is the proposal the CURRENT step evaluates:
// node 0 is always its sigma, however th1 arose); z: lane ST_ZLANE + i holds sigma's variate of the row i steps ahead (row of the
// current step: i == 0); par: s_par ([mu, scale, lb, ub][PIPE_KMAX]).  Real function on purpose: inline the pass tips the
// register allocation of the step loop (255 VGPRs, spill code inside the loop).  (The kernel switches the tree on for KIND 1 only,
// mh_mfma.hpp TREE; the reflective replay below ran the whole suite with the tree on everywhere and is what KIND 2 would use.)
typedef __attribute__((address_space(3))) double st_lds_d;   // LDS pointers stay LDS pointers across the call (ds_*, not flat_*)
template <int KIND>
__device__ __noinline__ void sigtree_build(st_lds_d* tab, const st_lds_d* par, double th0, double th1, double z, int k, int fixed, double dn) {
  const int lane = threadIdx.x & 63;
  const int d = 31 - __builtin_clz(lane + 1), path = lane + 1 - (1 << d);
  const double mu = par[0 * PIPE_KMAX + k - 1], sc = par[1 * PIPE_KMAX + k - 1];
  const double lb = par[2 * PIPE_KMAX + k - 1], ub = par[3 * PIPE_KMAX + k - 1];
  double a = readlane_d(th0, k - 1), b = readlane_d(th1, k - 1);
  // The replay is the pass's only loop and ran 24 instructions a level (round 7: the pass costs an owner ~1700 cycles, 6 % of the
  // step, profiles/r07_owner_window.md); now ten.  The increments of all levels come from ONE multiply and add, in the lanes that
  // hold the variates (the same doubles as mu + sc * z computed level by level).  The decisions of a lane sit left-aligned in
  // `take`: bit 31 - j is set where level j belongs to the lane's path AND accepts, so levels behind the lane's depth take nothing.
  // A fixed sigma skips the replay: its proposal is its state on every path (th1 == th0 in that lane, whatever the decisions).
  const double dzl = mu + sc * z;
  const unsigned take = ((unsigned)path << (31 - d)) << 1;
  if (!fixed) {
#pragma unroll
    for (int j = 0; j < ST_LOOK; j++) {            // decision j + 1 of the lane's path, then the owner's propose()
      const bool on = j < d;
      const double a1 = (take & (0x80000000u >> j)) ? b : a;
      double t = a1 + readlane_d(dzl, ST_ZLANE + j);
      if (KIND == FMCMC_KERNEL_NORMAL_REFLECTIVE) {
        if (on) t = reflect1(t, lb, ub);
      }
      a = a1;
      b = on ? t : b;
    }
  }
  const unsigned sg_hi = (unsigned)(fmh_d2u(b) >> 32);
  const bool sg_fast = (sg_hi - 0x00100000u) < 0x7fe00000u;                     // positive, finite, normal
  const double sg = sg_fast ? b : 1.0;
#ifdef MFO_NOLOG   /* timing ablation (tools/exp_mfmar.hip): what the logarithm costs */
  const double t1 = sg + FMH_K(FMH_LN_SQRT_2PI);
#else
  const double t1 = fmh_log_pn(sg) + FMH_K(FMH_LN_SQRT_2PI);                    // same bits as fmh_log(sigma) on this range
#endif
  const double ss = sg * sg;
  // denominator half of (0.5 tot) / sigma^2 (mh_common.hpp: div_recip / div_finish)
  const bool ok = sg_fast && mfr_div_safe(ss);
  const double rs = div_recip(ok ? ss : 1.0);
  typedef double st_d2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) st_d2 st_lds_d2;
  st_lds_d2* e = (st_lds_d2*)(tab + lane * ST_ENTRY);
  e[0] = st_d2{dn * t1, ss};
  e[1] = st_d2{rs, __longlong_as_double((long long)((sg_fast ? 1 : 0) | (ok ? 2 : 0)))};
}

}  // namespace

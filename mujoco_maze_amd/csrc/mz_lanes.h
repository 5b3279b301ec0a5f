// mz_lanes.h — the lane-group programming model the engines' dynamics headers are written in (ant_dyn.h, planar_dyn.h with
// point_bare.h, generic_dyn.h): one environment is advanced by a group of adjacent lanes of a wavefront, a phase is an
// MZ_FOR over independent items, cx.sync() is the hand-off between phases.
//
// Execution contexts (template parameter C):
//   * device: DevCtx of mz_device.h, instantiated by the kernels of csrc/ant_kernels.hip, planar_kernels.hip and
//     generic_kernels.hip — G lanes per env, cx.sync() = wavefront-scope fence, cx.gsum() = DPP/shuffle butterfly inside
//     the group;
//   * host emulation (HostCtx below; tests/emu, CPU tests of the kernel logic only — never a
//     product path): nlanes = 1, so every MZ_FOR runs all its items in order.
// Rule that makes both valid: inside one phase (between two cx.sync()) the
// iterations of an MZ_FOR are independent, and nothing but LDS scratch carries
// values from one phase to the next (group-uniform scalars may live in registers).
//
// Plain C++ (no HIP): shared by the kernel translation units and the CPU emulation in tests/emu/.
#pragma once

#if defined(__HIPCC__)
#define MZ_HD __host__ __device__ __forceinline__
#else
#define MZ_HD inline
#endif

#define MZ_FOR(i, n) for (int i = cx.lane0(); i < (n); i += C::nlanes)
// items 0..n-1 on the lanes base, base+1, ... (mod group size): lets unrelated work share one phase
#define MZ_FOR_AT(i, n, base) for (int i = mz_first_item(cx.lane0(), (base), C::nlanes); i < (n); i += C::nlanes)

MZ_HD int mz_first_item(int lane, int base, int nl) { return (lane - base) & (nl - 1); }  // group sizes are powers of two

struct HostCtx {
  static constexpr int nlanes = 1;
  static constexpr bool row_solver = false;  // the DPP-row Newton solver (ant_newton_rows.h) exists on the device only
  MZ_HD int lane0() const { return 0; }
  MZ_HD void sync() const {}
  MZ_HD float gsum(float x) const { return x; }
  MZ_HD double gsum(double x) const { return x; }
  MZ_HD double rowsum(double x) const { return x; }
  MZ_HD bool any(bool p) const { return p; }
  MZ_HD bool gany(bool p) const { return p; }
  MZ_HD unsigned long long gballot(bool p) const { return p ? 1ULL : 0ULL; }
  template <class S> MZ_HD void tick(S&, int) const {}
};

// Host-side launch helpers shared by every translation unit: grid sizes, the alignment and
// row-shape tests the launchers choose a kernel by, and the one dtype dispatch.
#pragma once
#include "fs2_common.h"

namespace {

inline unsigned nblk(long n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements of the activation dtype per 16 bytes (Vec<T>::N on the host side)
inline int vec_elems(int dtype) { return dtype == FS2_BF16 ? 8 : 4; }

// the vectorised row kernels: rows of D columns at a 16-byte aligned base and a
// row pitch of whole 16-byte vectors
inline bool vec_rows_ok(int dtype, int D, long ld, const void* p0, const void* p1) {
  const int vn = vec_elems(dtype);
  return D % vn == 0 && ld % vn == 0 && aligned16(p0) && aligned16(p1);
}
// column slabs of 64 lanes x one 16-byte vector
inline int slabs(int dtype, int D) { const int sc = 64 * vec_elems(dtype); return (D + sc - 1) / sc; }

// The dtype arms of a launcher, written once: f(bf16{}) or f(float{}) launches, with
// `using U = decltype(t)` naming the element type inside the generic lambda; any other dtype is
// refused before a launch.  Returns the launch status, so every entry point reports its own.
// (bf16 first: the order the kernels are instantiated in, and so their order in the code object.)
template <typename F>
int dispatch_dtype(int dtype, F&& f) {
  if (dtype == FS2_BF16) f(bf16{});
  else if (dtype == FS2_F32) f(float{});
  else return FS2_EINVAL;
  return (int)hipGetLastError();
}

}  // namespace

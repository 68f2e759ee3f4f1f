// Shared primitives of the data layer: the workgroup scan and reduction, the device-wide scan's pieces, the wave-aggregated
// append and the workspace carver that points.hip, text.hip, polygon.hip, track.hip, resample.hip, surface.hip and the tiff_*.hip files
// are built from.  Included by those files only: no training-path translation unit sees it (their look-alike scans and reductions are
// tuned in place).  Everything here is exact or order-fixed, so that a kernel built from it gives the same bytes from call to call.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>

// ---- wavefront ----
// the lanes of one wave hand bytes to each other through memory: order the wave's own stores before its later loads (host: one lane,
// nothing to order)
__host__ __device__ inline void lanes_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
}

// any trivially copyable T made of 32-bit words, shuffled word by word; a lane whose source lies outside the wave keeps its own value
template <class T, class Shfl>
__device__ __forceinline__ T wave_words(const T& v, Shfl shfl) {
  static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "shuffled in 32-bit words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = shfl(w[i]);
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
template <class T>
__device__ __forceinline__ T wave_shfl_up(const T& v, int off) {
  return wave_words(v, [off](int w) { return __shfl_up(w, off, 64); });
}
template <class T>
__device__ __forceinline__ T wave_shfl_down(const T& v, int off) {
  return wave_words(v, [off](int w) { return __shfl_down(w, off, 64); });
}

// Append to a list whose order is never visible: one atomic per wavefront.  Every lane of the wave calls it; the slot is valid where
// `keep` is.  Counter: unsigned or unsigned long long.
template <class Counter>
__device__ __forceinline__ Counter wave_append(bool keep, Counter* total) {
  const unsigned long long mask = __ballot(keep);
  if (mask == 0ull) return 0;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
  Counter at = 0;
  if (lane == leader) at = atomicAdd(total, (Counter)__popcll(mask));
  at = __shfl(at, leader, 64);
  return at + (Counter)__popcll(mask & ((1ull << lane) - 1ull));
}

// ---- workgroup scan (integers: wrapping sums, exact in any order) ----
// Exclusive scan of one T per thread over the NT threads of the workgroup; *total = the workgroup's sum, in every thread.  T has + and -
// and T{} is its zero.  Safe to call repeatedly: the trailing barrier frees wsum for the next call.
template <int NT, class T>
__device__ __forceinline__ T block_exscan(T v, T* total) {
  __shared__ T wsum[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const T o = wave_shfl_up(inc, off);
    if (lane >= off) inc = inc + o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  T base{}, tot{};
  for (int w = 0; w < NT / 64; ++w) {
    if (w < wave) base = base + wsum[w];
    tot = tot + wsum[w];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// The device-wide scan is three kernels: every workgroup sums its tile of NT * ITEMS items (scan_tile_items + block_exscan's total), one
// workgroup turns the tiles' sums into the sums in front of each tile (scan_parts), and the first kernel's work is done again with that
// base added.  Thread t of workgroup g owns the ITEMS consecutive items from scan_tile_first.
template <int NT, int ITEMS>
__device__ __forceinline__ long scan_tile_first() {
  return ((long)blockIdx.x * NT + (long)threadIdx.x) * ITEMS;
}

// k[j] = the calling thread's item j (zero at and beyond n); returns the sum of load(k[j]): what an item contributes is the caller's
template <int NT, int ITEMS, class T, class Item, class Load>
__device__ __forceinline__ T scan_tile_items(const Item* __restrict__ src, long n, Item* k, Load load) {
  const long first = scan_tile_first<NT, ITEMS>();
  T v{};
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    k[j] = first + j < n ? src[first + j] : Item(0);
    v = v + load(k[j]);
  }
  return v;
}

// one workgroup of NT threads: part[t] <- the sum of part[0 .. t) for every tile t; returns the sum of all (every thread)
template <int NT, class T>
__device__ __forceinline__ T scan_parts(T* part, long tiles) {
  T carry{};
  for (long t0 = 0; t0 < tiles; t0 += NT) {
    const long t = t0 + threadIdx.x;
    T tot;
    const T ex = block_exscan<NT>(t < tiles ? part[t] : T{}, &tot);
    if (t < tiles) part[t] = carry + ex;
    carry = carry + tot;
  }
  return carry;
}

// ---- workgroup reduction (floats: the order is the contract) ----
// One fixed tree: for off = 32 .. 1 the lanes below off take merge(own, the value of lane + off); thread 0 then folds the waves 1 ..
// NT / 64 - 1 in order.  merge(a, b) always gets the LOWER lane or wave as a: the float64 sums and Chan's merge of moments are not
// commutative in the last bit, and the results are specified bit for bit against restatements that walk this tree.  Valid in thread 0.
// AGAIN = true puts a barrier in front of the LDS write, so that a kernel may call it again while thread 0 may still be reading the
// words of the previous call (surface.hip's block_sum2); a kernel that calls it once leaves it out, as its own copy of the tree did.
template <int NT, bool AGAIN = false, class T, class Merge>
__device__ __forceinline__ T block_reduce(T v, Merge merge) {
  __shared__ T sh[NT / 64];
  for (int off = 32; off > 0; off >>= 1) {
    const T o = wave_shfl_down(v, off);
    if ((threadIdx.x & 63) < off) v = merge(v, o);
  }
  if (AGAIN) __syncthreads();   // (the words may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NT / 64; ++w) v = merge(v, sh[w]);
  return v;
}

// one workgroup finishes n partials: thread k folds load(k), load(k + NT), ... in order from `identity`, then the tree above
template <int NT, bool AGAIN = false, class T, class Load, class Merge>
__device__ __forceinline__ T fold_partials(long n, T identity, Load load, Merge merge) {
  T v = identity;
  for (long k = threadIdx.x; k < n; k += NT) v = merge(v, load(k));
  return block_reduce<NT, AGAIN>(v, merge);
}

// ---- host ----
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workgroups of a grid-stride launch over n items: at least one, at most max_blocks
inline int grid_stride_blocks(long n, int threads, int max_blocks) {
  const long b = (n + threads - 1) / threads;
  return (int)(b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

// Hands out 256-byte aligned arrays from a workspace.  A layout is written once, as a function on a Carver: on a null base it only
// measures (every take returns null), on the real base it carves; bytes() is what it has handed out either way.
struct Carver {
  char* base;
  size_t at = 0;
  explicit Carver(void* ws) : base((char*)ws) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + at) : nullptr;
    at += align256(sizeof(T) * count);
    return p;
  }
  size_t bytes() const { return at; }
};

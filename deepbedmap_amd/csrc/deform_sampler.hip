// Deformable convolution sampler (reference srgan_train.py:506-523, :572-574; Chainer deformable_convolution_2d_sampler +
// spatial_transformer_sampler semantics): the unfused half of the two deformable layers -- the sampler and its backward,
// the transposed sampling operator as CSR lists (built per (image, tap), gathered per input pixel), the 576 -> 1 GEMV.  The fused
// sampler + GEMM kernels are in deform_fwd.hip / deform_window.hip / deform_bwd.hip, the launch sequences of the layers in deform_layer.hip.  Order: helpers, the
// position-per-thread kernels, the list builder and its three kernels, the gathers, the launchers.
#include "dbm_internal.h"
#include "deform_geom.h"
#include "kernels.h"

// ---- the sampling lists: layout --------------------------------------------------------------------------------
// lists of (image n, tap t): offs[(n * 9 + t) * (plane + 1) + q] .. [q + 1] delimit the entries of input pixel q in
// ent[(n * 9 + t) * 4 * plane + ...] = {output position p, bilinear weight}, sorted by p (a fixed summation order);
// cur[(n * 9 + t) * plane + q]: the fill cursors of a build in global memory.
template <class T> __device__ __forceinline__ T* csr_offs_of(T* g_offs, int n, int t, int plane) { return g_offs + ((long)n * 9 + t) * (plane + 1); }
template <class T> __device__ __forceinline__ T* csr_ent_of(T* g_ent, int n, int t, int plane) { return g_ent + ((long)n * 9 + t) * 4 * plane; }
template <class T> __device__ __forceinline__ T* csr_cur_of(T* g_cur, int n, int t, int plane) { return g_cur + ((long)n * 9 + t) * plane; }

// The workspace that holds them, in floats from its start: the offsets, the 8-byte entries (8-byte aligned), then the cursors.
struct DeformCsrWorkspace {
  size_t ent_at, cur_at, end_at;
  DeformCsrWorkspace(int N, long plane)
      : ent_at(((size_t)N * 9 * (plane + 1) + 1) & ~(size_t)1), cur_at(ent_at + (size_t)N * 9 * 4 * plane * 2), end_at(cur_at + (size_t)N * 9 * plane) {}
  int* offs(float* ws) const { return (int*)ws; }
  int2* ent(float* ws) const { return (int2*)(ws + ent_at); }
  int* cur(float* ws) const { return (int*)(ws + cur_at); }
};

// ---- the LDS of the kernels that keep the lists of one (image, tap) there ----------------------------------------
// K channel planes, then the lists: plane + 1 offsets, plane cursors, 4 * plane entries of 8 bytes.
constexpr size_t DEFORM_LDS_BUDGET = 150 * 1024;   // what a plane may ask for
constexpr int DEFORM_LDS_ATTR = 152 * 1024;        // the limit the kernels are given: the budget and some room for their static wtot[]
static size_t deform_lds_bytes(int K, long plane) { return sizeof(float) * ((size_t)K * plane + 10 * (size_t)plane + 1); }

// col[n][c*9+t][p] = bilinear sample of x[n][c] at (tap t position + offset)
__global__ __launch_bounds__(256) void deform_sample_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                            float* __restrict__ col, int N, int C, int H, int W,
                                                            long offsn) {
  const int plane = H * W;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * 9 * plane) return;
  const int p = (int)(e % plane);
  const int t = (int)((e / plane) % 9);
  const int n = (int)(e / (9L * plane));
  const DeformTap s = deform_tap(off + (long)n * offsn, t, p, H, W);
  const float* xn = x + (long)n * C * plane;
  float* cn = col + ((long)n * C * 9 + t) * plane + p;
  for (int c = 0; c < C; ++c) {
    const float* xc = xn + (long)c * plane;
    const float x1 = s.o1 >= 0 ? xc[s.o1] : 0.f, x2 = s.o2 >= 0 ? xc[s.o2] : 0.f;
    const float x3 = s.o3 >= 0 ? xc[s.o3] : 0.f, x4 = s.o4 >= 0 ? xc[s.o4] : 0.f;
    cn[(long)c * 9 * plane] = s.w1() * x1 + s.w2() * x2 + s.w3() * x3 + s.w4() * x4;
  }
}

// Backward of the sampler.  gcol[n][c*9+t][p] is either read (gcol != null) or, for a single
// output channel, formed on the fly as w1o[c*9+t] * gy[n][p].  Scatters into gx (atomics; gx
// must be zero-initialised or hold the gradient it accumulates onto) and writes goff[n][0:18].
__global__ __launch_bounds__(256) void deform_backward_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                              const float* __restrict__ gcol,
                                                              const float* __restrict__ w1o,
                                                              const float* __restrict__ gy, float* gx,
                                                              float* __restrict__ goff, int N, int C, int H, int W,
                                                              long offsn) {
  const int plane = H * W;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * 9 * plane) return;
  const int p = (int)(e % plane);
  const int t = (int)((e / plane) % 9);
  const int n = (int)(e / (9L * plane));
  const DeformTap s = deform_tap(off + (long)n * offsn, t, p, H, W);
  const float* xn = x + (long)n * C * plane;
  float* gxn = gx + (long)n * C * plane;
  const float gyv = gy ? gy[(long)n * plane + p] : 0.f;
  float gu = 0.f, gv = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* xc = xn + (long)c * plane;
    float* gxc = gxn + (long)c * plane;
    const float gq = gcol ? gcol[((long)n * C * 9 + (long)c * 9 + t) * plane + p] : w1o[c * 9 + t] * gyv;
    const float x1 = s.o1 >= 0 ? xc[s.o1] : 0.f, x2 = s.o2 >= 0 ? xc[s.o2] : 0.f;
    const float x3 = s.o3 >= 0 ? xc[s.o3] : 0.f, x4 = s.o4 >= 0 ? xc[s.o4] : 0.f;
    float du, dv;
    deform_coord_grads(s.g, x1, x2, x3, x4, du, dv);
    gu += gq * du;
    gv += gq * dv;
    if (s.o1 >= 0) atomicAdd(gxc + s.o1, gq * s.w1());
    if (s.o2 >= 0) atomicAdd(gxc + s.o2, gq * s.w2());
    if (s.o3 >= 0) atomicAdd(gxc + s.o3, gq * s.w3());
    if (s.o4 >= 0) atomicAdd(gxc + s.o4, gq * s.w4());
  }
  float* gn = goff + (long)n * offsn;
  gn[(long)t * plane + p] = s.g.mu ? gu : 0.f;
  gn[(long)(9 + t) * plane + p] = s.g.mv ? gv : 0.f;
}

// Offset gradients without atomics (deterministic mode): one thread per (image, tap, position) walks all channels.
__global__ __launch_bounds__(256) void deform_goff_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                          const float* __restrict__ gcol, const float* __restrict__ w1o,
                                                          const float* __restrict__ gy, float* __restrict__ goff, int N, int C,
                                                          int H, int W, long offsn) {
  const int plane = H * W;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * 9 * plane) return;
  const int p = (int)(e % plane);
  const int t = (int)((e / plane) % 9);
  const int n = (int)(e / (9L * plane));
  const DeformTap s = deform_tap(off + (long)n * offsn, t, p, H, W);
  const float* xn = x + (long)n * C * plane;
  const float gyv = gy ? gy[(long)n * plane + p] : 0.f;
  float gu = 0.f, gv = 0.f;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const float* xc = xn + (long)c * plane;
    const float gq = gcol ? gcol[((long)n * C * 9 + (long)c * 9 + t) * plane + p] : w1o[c * 9 + t] * gyv;
    const float x1 = s.o1 >= 0 ? xc[s.o1] : 0.f, x2 = s.o2 >= 0 ? xc[s.o2] : 0.f;
    const float x3 = s.o3 >= 0 ? xc[s.o3] : 0.f, x4 = s.o4 >= 0 ? xc[s.o4] : 0.f;
    float du, dv;
    deform_coord_grads(s.g, x1, x2, x3, x4, du, dv);
    gu += gq * du;
    gv += gq * dv;
  }
  float* gn = goff + (long)n * offsn;
  gn[(long)t * plane + p] = s.g.mu ? gu : 0.f;
  gn[(long)(9 + t) * plane + p] = s.g.mv ? gv : 0.f;
}

// ---- the list builder ------------------------------------------------------------------------------------------
// The sampling pattern of a tap is shared by all channels, so the scatter of the sampler's backward is done as a gather: per (image,
// tap) a workgroup builds the TRANSPOSED sparse sampling operator -- a CSR list, per input pixel q, of the output positions p and
// bilinear weights that touch q (counting sort with integer atomics) -- and every channel then sums gx[c][q] over list(q), each q
// owned by one lane (fp32 atomics on gx retire about one lane per clock).
//
// Where the lists of one (image, tap) are while they are built is a storage policy: counts-then-offsets `offs` (plane + 1), fill cursors
// `cur` (plane), entries get / put as {position, weight bits}, end_phase() between a phase that writes and one that reads, and which
// gaps the sort of its lists takes (csr_sort_list).
struct CsrInLds {   // entries as two arrays of 4 * plane; a barrier orders LDS
  int* offs;
  int* cur;
  int* ent_p;
  float* ent_w;
  __device__ __forceinline__ CsrInLds(float* at, int plane)
      : offs((int*)at), cur(offs + plane + 1), ent_p(cur + plane), ent_w((float*)(ent_p + 4 * plane)) {}
  __device__ __forceinline__ int2 get(int i) const { return make_int2(ent_p[i], __float_as_int(ent_w[i])); }
  __device__ __forceinline__ void put(int i, int2 e) const { ent_p[i] = e.x; ent_w[i] = __int_as_float(e.y); }
  __device__ __forceinline__ void end_phase() const { __syncthreads(); }
  static constexpr bool kShellSort = false;
};
struct CsrInGlobal {   // the workspace's own arrays; the counts and cursors are written by atomics (performed in L2) and read by plain
  int* offs;           // loads, so a device-scope fence goes before the barrier
  int* cur;
  int2* ent;
  __device__ __forceinline__ int2 get(int i) const { return ent[i]; }
  __device__ __forceinline__ void put(int i, int2 e) const { ent[i] = e; }
  __device__ __forceinline__ void end_phase() const { __threadfence(); __syncthreads(); }
  static constexpr bool kShellSort = true;
};

// The fill order (cursor atomics) varies from run to run, so a list is sorted by position before it is summed.  A position occurs at
// most once in a pixel's list (the four corners of a sample are four different pixels), so the sorted list is unique whatever the
// algorithm.  One loop, its gaps chosen by the storage policy: in global memory a Shell sort (gaps 3h + 1: no quadratic walk where many
// samples converge on one pixel of a plane of any size); in LDS, where a list has at most `plane` <= 3839 entries and usually a
// handful, the single gap 1 -- the insertion sort.  The Shell sort's gap bookkeeping there made deform_csr_build_kernel, which runs
// twice per training iteration, 40 instead of 34 us (profiles/r7/deform_sampler_refactor.txt).
template <class Store>
__device__ __forceinline__ void csr_sort_list(const Store& st, int s0, int s1) {
  int h = 1;
  if constexpr (Store::kShellSort)
    while (h < (s1 - s0) / 3) h = 3 * h + 1;
  for (; h >= 1; h /= 3)
    for (int i = s0 + h; i < s1; ++i) {
      const int2 k = st.get(i);
      int jj = i;
      while (jj - h >= s0 && st.get(jj - h).x > k.x) {
        st.put(jj, st.get(jj - h));
        jj -= h;
      }
      st.put(jj, k);
    }
}

// Count, exclusive scan, fill, and (SORT) sort by position, by the NT threads of a workgroup for tap t of the image whose offset planes
// are `on`.  wtot: NT / 64 ints of LDS.  at_fill(p, tap) is called once per position in the fill pass, for a caller that has more to do
// with a sample's geometry.  On return list(q) is complete -- and sorted -- for the thread that sorted it, the one with q % NT == tid: a
// caller whose threads read other lists than their own ends the phase first.
template <int NT, bool SORT, class Store, class AtFill>
__device__ __forceinline__ void deform_build_lists(const Store& st, const float* __restrict__ on, int t, int H, int W, int* wtot, AtFill at_fill) {
  const int plane = H * W, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e <= plane; e += NT) st.offs[e] = 0;
  st.end_phase();
  // ---- pass 1: how many samples touch each input pixel ----
  for (int p = tid; p < plane; p += NT) {
    const DeformTap s = deform_tap(on, t, p, H, W);
    if (s.o1 >= 0) atomicAdd(st.offs + s.o1, 1);
    if (s.o2 >= 0) atomicAdd(st.offs + s.o2, 1);
    if (s.o3 >= 0) atomicAdd(st.offs + s.o3, 1);
    if (s.o4 >= 0) atomicAdd(st.offs + s.o4, 1);
  }
  st.end_phase();
  // ---- exclusive scan of the counts: each thread owns `per` consecutive ones (tid * per < plane + NT: no overflow) ----
  {
    const int per = (plane + NT - 1) / NT;
    const int base = tid * per;
    int loc = 0;
    for (int i = 0; i < per; ++i)
      if (base + i < plane) loc += st.offs[base + i];
    int inc = loc;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int pre = inc - loc;
    for (int w2 = 0; w2 < wave; ++w2) pre += wtot[w2];
    for (int i = 0; i < per; ++i)
      if (base + i < plane) {
        const int cnt = st.offs[base + i];
        st.offs[base + i] = pre;
        st.cur[base + i] = pre;
        pre += cnt;
      }
    if (tid == NT - 1) st.offs[plane] = pre;  // the last thread owns the tail (possibly empty): pre == grand total
  }
  st.end_phase();
  // ---- pass 2: fill the lists ----
  for (int p = tid; p < plane; p += NT) {
    const DeformTap s = deform_tap(on, t, p, H, W);
    if (s.o1 >= 0) st.put(atomicAdd(st.cur + s.o1, 1), make_int2(p, __float_as_int(s.w1())));
    if (s.o2 >= 0) st.put(atomicAdd(st.cur + s.o2, 1), make_int2(p, __float_as_int(s.w2())));
    if (s.o3 >= 0) st.put(atomicAdd(st.cur + s.o3, 1), make_int2(p, __float_as_int(s.w3())));
    if (s.o4 >= 0) st.put(atomicAdd(st.cur + s.o4, 1), make_int2(p, __float_as_int(s.w4())));
    at_fill(p, s);
  }
  st.end_phase();
  if constexpr (SORT)
    for (int q = tid; q < plane; q += NT) csr_sort_list(st, st.offs[q], st.offs[q + 1]);
}

// Lists built in LDS and copied out: g_offs / g_ent of DeformCsrWorkspace.
template <int NT>
__global__ __launch_bounds__(NT) void deform_csr_build_kernel(const float* __restrict__ off, int* __restrict__ g_offs,
                                                              int2* __restrict__ g_ent, int H, int W, long offsn) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ int wtot[NT / 64];
  const int plane = H * W;
  const int n = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const CsrInLds st(sm, plane);
  deform_build_lists<NT, true>(st, off + (long)n * offsn, t, H, W, wtot, [](int, const DeformTap&) {});
  int* go = csr_offs_of(g_offs, n, t, plane);
  int2* ge = csr_ent_of(g_ent, n, t, plane);
  for (int q = tid; q < plane; q += NT) {   // (each thread the lists it sorted)
    const int s0 = st.offs[q], s1 = st.offs[q + 1];
    go[q] = s0;
    for (int sl = s0; sl < s1; ++sl) ge[sl] = st.get(sl);
  }
  if (tid == 0) go[plane] = st.offs[plane];
}

// The same lists for a plane of any size (launch_deform_backward's deterministic form past the LDS kernels): counts, offsets, cursors
// and entries all live in global memory, one workgroup per (image, tap), sorted in place.
template <int NT>
__global__ __launch_bounds__(NT) void deform_csr_build_global_kernel(const float* __restrict__ off, int* g_offs, int2* g_ent, int* g_cur,
                                                                     int H, int W, long offsn) {
  __shared__ int wtot[NT / 64];
  const int plane = H * W;
  const int n = blockIdx.x, t = blockIdx.y;
  const CsrInGlobal st{csr_offs_of(g_offs, n, t, plane), csr_cur_of(g_cur, n, t, plane), csr_ent_of(g_ent, n, t, plane)};
  deform_build_lists<NT, true>(st, off + (long)n * offsn, t, H, W, wtot, [](int, const DeformTap&) {});
}

// ---- the gathers -----------------------------------------------------------------------------------------------
// One list entry {p, w} of (image n, tap t) into the sums of channels c0 .. c0 + CH of an input pixel: acc[c] += w * gcol[c0 + c][t][p]
// (gc0 = that plane of channel c0), or without a column-gradient matrix (gc0 null: a single output channel) w * gy[n][p] * w1o[(c0 + c) * 9 + t].
// The CH loads of an entry are independent and in flight together.  (Which of these multiply-adds the compiler contracts decides the last
// bit of gx: a change here is checked against the previous build bit for bit, profiles/r7/deform_sampler_refactor.txt.)
template <int CH>
__device__ __forceinline__ void deform_gather_entry(float (&acc)[CH], int p, float w, const float* __restrict__ gc0,
                                                    const float* __restrict__ gy, const float* __restrict__ w1o, int n, int c0, int t,
                                                    int plane) {
  if (gc0) {
    float gq[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) gq[c] = gc0[(long)c * 9 * plane + p];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] += w * gq[c];
  } else {
    const float gyv = w * gy[(long)n * plane + p];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] += gyv * w1o[(c0 + c) * 9 + t];
  }
}

// Lists and gather in one kernel: a workgroup per (image, CH channels) rebuilds the lists of each tap in LDS and sums into CH channel
// planes there.  gx is overwritten.  DET: the lists are sorted and x is not staged -- the offset gradients, its only reader, come from
// deform_goff_kernel (no atomics across channel groups), which leaves room for 16 channels per workgroup.  !DET: the offset gradients are
// added to goff (zeroed by the caller) in the fill pass, a gather already: 4 corner reads per channel.
template <int CH, int NT, bool DET>
__global__ __launch_bounds__(NT) void deform_backward_csr_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                                  const float* __restrict__ gcol,
                                                                  const float* __restrict__ w1o,
                                                                  const float* __restrict__ gy, float* __restrict__ gx,
                                                                  float* goff, int N, int C, int H, int W, long offsn) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ int wtot[NT / 64];
  const int plane = H * W;
  float* sx = sm;                              // CH * plane (not in the DET variant)
  float* sg = DET ? sm : sx + CH * plane;      // CH * plane
  const CsrInLds st(sg + CH * plane, plane);
  const int n = blockIdx.x, c0 = blockIdx.y * CH, tid = threadIdx.x;
  const float* xn = x + ((long)n * C + c0) * plane;
  for (int e = tid; e < CH * plane; e += NT) {
    if constexpr (!DET) sx[e] = xn[e];
    sg[e] = 0.f;
  }
  float* gn = goff + (long)n * offsn;
  for (int t = 0; t < 9; ++t) {
    deform_build_lists<NT, DET>(st, off + (long)n * offsn, t, H, W, wtot, [&](int p, const DeformTap& s) {
      if constexpr (!DET) {
        const float gyv = gy ? gy[(long)n * plane + p] : 0.f;
        float gu = 0.f, gv = 0.f;
        float gqs[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c)
          gqs[c] = gcol ? gcol[((long)n * C * 9 + (long)(c0 + c) * 9 + t) * plane + p] : w1o[(c0 + c) * 9 + t] * gyv;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float* xc = sx + c * plane;
          const float x1 = s.o1 >= 0 ? xc[s.o1] : 0.f, x2 = s.o2 >= 0 ? xc[s.o2] : 0.f;
          const float x3 = s.o3 >= 0 ? xc[s.o3] : 0.f, x4 = s.o4 >= 0 ? xc[s.o4] : 0.f;
          float du, dv;
          deform_coord_grads(s.g, x1, x2, x3, x4, du, dv);
          gu += gqs[c] * du;
          gv += gqs[c] * dv;
        }
        if (s.g.mu) atomicAdd(gn + (long)t * plane + p, gu);
        if (s.g.mv) atomicAdd(gn + (long)(9 + t) * plane + p, gv);
      }
    });
    // ---- gather: every input pixel q sums its list (entries outer, channels inner) ----
    const float* gc0 = gcol ? gcol + ((long)n * C * 9 + (long)c0 * 9 + t) * plane : nullptr;
    for (int q = tid; q < plane; q += NT) {
      float acc[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = 0.f;
      for (int sl = st.offs[q], s1 = st.offs[q + 1]; sl < s1; ++sl) {
        const int2 en = st.get(sl);
        deform_gather_entry<CH>(acc, en.x, __int_as_float(en.y), gc0, gy, w1o, n, c0, t, plane);
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) sg[c * plane + q] += acc[c];
    }
    __syncthreads();
  }
  float* gxn = gx + ((long)n * C + c0) * plane;
  for (int e = tid; e < CH * plane; e += NT) gxn[e] = sg[e];
}

// The same gather from stored lists (built ONCE per (image, tap) where the kernel above rebuilds them in each of the C / CH workgroups of
// an image): gx[n][c0 .. c0 + CH)[q] = sum over taps and list entries; input pixel q owned by one thread, its CH sums in registers over
// all nine taps, no LDS.
template <int CH, int NT>
__global__ __launch_bounds__(NT) void deform_csr_gather_kernel(const int* __restrict__ g_offs, const int2* __restrict__ g_ent,
                                                               const float* __restrict__ gcol, const float* __restrict__ w1o,
                                                               const float* __restrict__ gy, float* __restrict__ gx, int C, int plane) {
  const int n = blockIdx.x, c0 = blockIdx.y * CH;
  for (int q = threadIdx.x; q < plane; q += NT) {
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.f;
    for (int t = 0; t < 9; ++t) {
      const int* go = csr_offs_of(g_offs, n, t, plane);
      const int2* ge = csr_ent_of(g_ent, n, t, plane);
      const int s0 = go[q], s1 = go[q + 1];
      const float* gc0 = gcol ? gcol + (((long)n * C + c0) * 9 + t) * plane : nullptr;
      for (int sl = s0; sl < s1; ++sl) {
        const int2 en = ge[sl];
        deform_gather_entry<CH>(acc, en.x, __int_as_float(en.y), gc0, gy, w1o, n, c0, t, plane);
      }
    }
    float* gxn = gx + ((long)n * C + c0) * plane + q;
#pragma unroll
    for (int c = 0; c < CH; ++c) gxn[(long)c * plane] = acc[c];
  }
}

// G[n][t][q] = sum over the list entries of input pixel q of w * gy[n][p]: the transposed sampler applied to ONE value per position and
// tap (the 64 -> 1 layer's backward in premultiplied form, deform_bwd.hip); one thread per (image, tap, input pixel).
__global__ __launch_bounds__(256) void deform_csr_gather1_kernel(const int* __restrict__ g_offs, const int2* __restrict__ g_ent,
                                                                 const float* __restrict__ gy, float* __restrict__ G, int plane) {
  const int n = blockIdx.z, t = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= plane) return;
  const int* go = csr_offs_of(g_offs, n, t, plane);
  const int2* ge = csr_ent_of(g_ent, n, t, plane);
  const float* gyn = gy + (long)n * plane;
  const int s0 = go[q], s1 = go[q + 1];
  float acc = 0.f;
  for (int sl = s0; sl < s1; ++sl) {   // (entries sorted by position: a fixed summation order)
    const int2 en = ge[sl];
    acc += __int_as_float(en.y) * gyn[en.x];
  }
  G[((long)n * 9 + t) * plane + q] = acc;
}

// ---- launchers -------------------------------------------------------------------------------------------------
void launch_deform_sample(const float* x, const float* off, float* col, int N, int C, int H, int W, long offsn,
                          hipStream_t s) {
  const long total = (long)N * 9 * H * W;
  hipLaunchKernelGGL(deform_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, off, col, N, C,
                     H, W, offsn);
  DBM_HIP(hipGetLastError());
}

static void deform_lds_attributes() {   // the three kernels with lists in LDS: once per process
  static bool set = false;
  if (set) return;
  DBM_HIP(hipFuncSetAttribute((const void*)deform_backward_csr_kernel<8, 1024, false>, hipFuncAttributeMaxDynamicSharedMemorySize, DEFORM_LDS_ATTR));
  DBM_HIP(hipFuncSetAttribute((const void*)deform_backward_csr_kernel<16, 1024, true>, hipFuncAttributeMaxDynamicSharedMemorySize, DEFORM_LDS_ATTR));
  DBM_HIP(hipFuncSetAttribute((const void*)deform_csr_build_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, DEFORM_LDS_ATTR));
  set = true;
}

size_t deform_csr_workspace_floats(int N, int H, int W) { return DeformCsrWorkspace(N, (long)H * W).cur_at; }

// (the plane fits the kernels that keep the sampling lists of one (image, tap) and sixteen channel planes in LDS: x and gx of eight
//  channels, or gx of sixteen in deterministic mode -- planes up to 1476 positions)
static bool deform_backward_lds_ok(int C, long plane) { return C % 8 == 0 && deform_lds_bytes(16, plane) <= DEFORM_LDS_BUDGET; }

// Floats of list workspace launch_deform_backward needs (0: none): in deterministic mode a plane past the LDS kernels builds its
// sampling lists in global memory -- the lists, then the fill cursors.
size_t deform_backward_workspace_floats(int N, int C, int H, int W) {
  const long plane = (long)H * W;
  if (!g_wgrad_deterministic || C % 8 != 0 || deform_backward_lds_ok(C, plane)) return 0;
  return DeformCsrWorkspace(N, plane).end_at;
}

// gx is fully overwritten; goff[n][0:18] is overwritten (channels 18.. of a padded offset tensor are left alone).
// ws: deform_backward_workspace_floats floats (may be null where that is 0).
void launch_deform_backward(const float* x, const float* off, const float* gcol, const float* w1o, const float* gy,
                            float* gx, float* goff, int N, int C, int H, int W, long offsn, hipStream_t s, float* ws) {
  const long plane = (long)H * W;
  const long total = (long)N * 9 * plane;
  const bool lds = deform_backward_lds_ok(C, plane);
  if (g_wgrad_deterministic && C % 8 == 0) {
    // No fp32 atomics on a plane of any size: the offset gradients from deform_goff_kernel, then sorted lists and a gather per 16 channels
    DBM_CHECK(C % 16 == 0, "deformable backward: the deterministic forms take 16 channels per workgroup (dbm_op_deform_conv2d_backward: C % 32 == 0)");
    hipLaunchKernelGGL(deform_goff_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, off, gcol, w1o, gy, goff, N, C,
                       H, W, offsn);
    if (lds) {   // one round of N * C / 16 workgroups, each with the lists in LDS
      deform_lds_attributes();
      hipLaunchKernelGGL((deform_backward_csr_kernel<16, 1024, true>), dim3(N, C / 16), dim3(1024), deform_lds_bytes(16, plane), s, x, off,
                         gcol, w1o, gy, gx, goff, N, C, H, W, offsn);
    } else {     // the lists of every (image, tap) built and sorted in global memory, then the register-only gather
      DBM_CHECK(ws != nullptr, "deformable backward: the deterministic form past the LDS kernels needs deform_backward_workspace_floats of workspace");
      DBM_CHECK(4 * plane < (1L << 31), "deformable backward: more than 2^29 pixels per plane");
      const DeformCsrWorkspace l(N, plane);
      hipLaunchKernelGGL((deform_csr_build_global_kernel<1024>), dim3(N, 9), dim3(1024), 0, s, off, l.offs(ws), l.ent(ws), l.cur(ws), H, W, offsn);
      hipLaunchKernelGGL((deform_csr_gather_kernel<16, 1024>), dim3(N, C / 16), dim3(1024), 0, s, l.offs(ws), l.ent(ws), gcol, w1o, gy, gx, C,
                         (int)plane);
    }
  } else if (lds) {
    deform_lds_attributes();
    DBM_HIP(hipMemset2DAsync(goff, sizeof(float) * offsn, 0, sizeof(float) * 18 * plane, N, s));
    hipLaunchKernelGGL((deform_backward_csr_kernel<8, 1024, false>), dim3(N, C / 8), dim3(1024), deform_lds_bytes(16, plane), s, x, off, gcol,
                       w1o, gy, gx, goff, N, C, H, W, offsn);
  } else {
    DBM_HIP(hipMemsetAsync(gx, 0, sizeof(float) * N * C * plane, s));
    hipLaunchKernelGGL(deform_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, off, gcol, w1o,
                       gy, gx, goff, N, C, H, W, offsn);
  }
  DBM_HIP(hipGetLastError());
}

// Input gradient only: the CSR gather from stored lists, without the offset gradients (which the fused kernels of deform_bwd.hip
// produce).  False when a plane does not fit (the caller then takes launch_deform_backward).  The limit counts eight channel planes of
// LDS beside the lists, which the register-only gather no longer uses: that is where the 2133 positions come from (the lists alone,
// deform_csr_lists_ok, fit up to 3839).  It stays: it decides which kernels run.
bool deform_input_grad_ok(int C, int H, int W) { return C % 8 == 0 && deform_lds_bytes(8, (long)H * W) <= DEFORM_LDS_BUDGET; }

bool deform_csr_lists_ok(int C, int H, int W) { return C % 16 == 0 && deform_lds_bytes(0, (long)H * W) <= DEFORM_LDS_BUDGET; }

void launch_deform_csr_build(const float* off, float* ws, int N, int H, int W, long offsn, hipStream_t s) {
  const long plane = (long)H * W;
  DBM_CHECK(ws != nullptr && deform_lds_bytes(0, plane) <= DEFORM_LDS_BUDGET, "deformable CSR lists: plane too large");
  const DeformCsrWorkspace l(N, plane);
  deform_lds_attributes();
  hipLaunchKernelGGL((deform_csr_build_kernel<1024>), dim3(N, 9), dim3(1024), deform_lds_bytes(0, plane), s, off, l.offs(ws), l.ent(ws), H, W,
                     offsn);
  DBM_HIP(hipGetLastError());
}

// ws: deform_csr_workspace_floats floats -- the sampling lists are built once per (image, tap) there (unless `lists_built`), then a
// register-only kernel gathers per (image, 16 channels)
void launch_deform_input_grad(const float* off, const float* gcol, const float* w1o, const float* gy, float* gx, int N, int C, int H, int W,
                              long offsn, hipStream_t s, float* ws, bool lists_built) {
  DBM_CHECK(deform_input_grad_ok(C, H, W), "deformable input gradient: plane too large for the CSR kernel");
  DBM_CHECK(ws && deform_csr_lists_ok(C, H, W), "deformable input gradient: needs a list workspace and C % 16 == 0");
  const long plane = (long)H * W;
  const DeformCsrWorkspace l(N, plane);
  if (!lists_built) launch_deform_csr_build(off, ws, N, H, W, offsn, s);
  hipLaunchKernelGGL((deform_csr_gather_kernel<16, 1024>), dim3(N, C / 16), dim3(1024), 0, s, l.offs(ws), l.ent(ws), gcol, w1o, gy, gx, C,
                     (int)plane);
  DBM_HIP(hipGetLastError());
}

// The sampling lists of `off` (built into ws) applied to gy (N, 1, plane): G (N, 9, plane).
void launch_deform_csr_gather1(const float* off, const float* gy, float* G, int N, int H, int W, long offsn, hipStream_t s, float* ws,
                               bool lists_built) {
  const long plane = (long)H * W;
  DBM_CHECK(ws != nullptr && deform_lds_bytes(0, plane) <= DEFORM_LDS_BUDGET, "deformable CSR lists: plane too large");
  const DeformCsrWorkspace l(N, plane);
  if (!lists_built) launch_deform_csr_build(off, ws, N, H, W, offsn, s);
  hipLaunchKernelGGL(deform_csr_gather1_kernel, dim3((unsigned)((plane + 255) / 256), 9, N), dim3(256), 0, s, l.offs(ws), l.ent(ws), gy, G,
                     (int)plane);
  DBM_HIP(hipGetLastError());
}

// y[n][0][p] = b + sum_k w[k] * col[n][k][p]   (final_conv_layer2's 576 -> 1 GEMV, srgan_train.py:574)
__global__ __launch_bounds__(256) void gemv_cols_kernel(const float* __restrict__ col, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int N,
                                                        int K, int plane) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * plane) return;
  const int n = (int)(e / plane), p = (int)(e - (long)n * plane);
  const float* c = col + (long)n * K * plane + p;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = 0;
  for (; k + 3 < K; k += 4) {
    a0 = fmaf(w[k], c[(long)k * plane], a0);
    a1 = fmaf(w[k + 1], c[(long)(k + 1) * plane], a1);
    a2 = fmaf(w[k + 2], c[(long)(k + 2) * plane], a2);
    a3 = fmaf(w[k + 3], c[(long)(k + 3) * plane], a3);
  }
  for (; k < K; ++k) a0 = fmaf(w[k], c[(long)k * plane], a0);
  y[e] = (a0 + a1) + (a2 + a3) + (bias ? bias[0] : 0.f);
}

void launch_gemv_cols(const float* col, const float* w, const float* bias, float* y, int N, int K, int plane,
                      hipStream_t s) {
  const long total = (long)N * plane;
  hipLaunchKernelGGL(gemv_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, col, w, bias, y, N, K,
                     plane);
  DBM_HIP(hipGetLastError());
}

// gw[k] += sum_{n,p} gy[n][p] * col[n][k][p];  gb += sum gy     (backward of the GEMV above)
// One 1024-thread workgroup per k: one wavefront per image at a time, lanes along the plane; fixed-order tree, no
// fp32 atomics (reproducible).
__global__ __launch_bounds__(1024) void gemv_cols_wgrad_kernel(const float* __restrict__ col,
                                                               const float* __restrict__ gy, float* gw, float* gb,
                                                               int N, int K, int plane) {
  __shared__ float part[16];
  const int k = blockIdx.x;  // k == K computes the bias gradient
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f;
  for (int n = wave; n < N; n += 16) {
    const float* g = gy + (long)n * plane;
    const float* c = col + ((long)n * K + (k < K ? k : 0)) * plane;
    for (int p = lane; p < plane; p += 64) acc += g[p] * (k < K ? c[p] : 1.f);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int w = 0; w < 16; ++w) v += part[w];
    if (k < K) gw[k] += v;
    else if (gb) gb[0] += v;
  }
}

void launch_gemv_cols_wgrad(const float* col, const float* gy, float* gw, float* gb, int N, int K, int plane,
                            hipStream_t s) {
  hipLaunchKernelGGL(gemv_cols_wgrad_kernel, dim3(K + 1), dim3(1024), 0, s, col, gy, gw, gb, N, K, plane);
  DBM_HIP(hipGetLastError());
}

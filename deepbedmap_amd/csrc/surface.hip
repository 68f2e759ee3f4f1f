// Tension-spline surface through the constraint nodes of a raster (reference data_prep.py:410-419: `gmt.surface(T=0.35, M="3c")`; the
// definition and what differs from GMT: DESIGN.md "Tension surface", include/dbm.h).  With NaN nodes free (F) and every other node a
// constraint (K), the output minimises
//   E(u) = (1 - T) (sum sxx^2 + sum syy^2 + 2 sum sxy^2) + T (sum sx^2 + sum sy^2),   u = d on K,
// over the differences whose stencil fits inside the grid (sxx[r, c] = u[r, c-1] - 2 u[r, c] + u[r, c+1] for 1 <= c <= W-2, syy alike,
// sxy[r, c] = u[r+1, c+1] - u[r+1, c] - u[r, c+1] + u[r, c] for r <= H-2, c <= W-2, sx, sy first differences): the plate's natural free
// edge, no ghost rows.  A = (1 - T)(Dxx' Dxx + Dyy' Dyy + 2 Dxy' Dxy) + T (Dx' Dx + Dy' Dy); A_FF x = b = -[A (d - m on K, 0 on F)]_F is
// solved in float64 by Jacobi-preconditioned conjugate gradients from x = 0, m the first constraint node's value (row-major).
//
// Vectors are full-grid float64 arrays that are zero on K, so A_FF p = mask . A(mask . p) and one operator kernel serves b and the
// iterations.  Three launches per iteration:
//   surface_operator_kernel   Ap = mask . A p from a 16 x 64 tile of p staged in LDS with a halo of two nodes; p . Ap per tile;
//                             the last tile to arrive (integer ticket) folds the partials in tile order and forms alpha
//   surface_update_kernel     x += alpha p, r -= alpha Ap, z = r / diag; r . z and r . r per workgroup; the last workgroup forms beta,
//                             counts the iteration and raises `done` when |r| <= tol |b|
//   surface_direction_kernel  p = z + beta p
// Every kernel returns at once when `done` is up, so the host may enqueue 32 iterations before it reads the state back.  No float
// atomics; launch shapes depend on H and W only: the same bytes from call to call.
#include "model.h"
#include "data_layouts.h"
#include <cmath>

namespace {

constexpr int SURF_THREADS = 256;
constexpr int SURF_TR = 16, SURF_TC = 64;   // the operator's tile: one wavefront per row of 64 nodes, four rows per thread
constexpr int SURF_HALO = 2;
constexpr int SURF_LR = SURF_TR + 2 * SURF_HALO, SURF_LC = SURF_TC + 2 * SURF_HALO;   // 20 x 68 doubles = 10 880 bytes of LDS
constexpr int SURF_MAX_BLOCKS = 2048;       // the elementwise kernels: 8 workgroups per CU, grid-stride beyond
constexpr int SURF_CHECK_EVERY = 32;        // iterations enqueued between two reads of the state

struct SurfState {   // device; zero when the call begins
  double rz, pap, alpha, beta, rr, bb, tol2bb;
  unsigned first_inv;    // max over the constraint nodes of ~index: ~first_inv is the lowest row-major constraint index
  unsigned constraints;
  int done, iters;
  unsigned ticket[2];
};

__device__ inline void store_agent(double* p, double v) {   // write-through: read by another workgroup of the same launch
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline double load_agent(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
}

// two sums that travel through one reduction tree (block_reduce: valid in thread 0)
struct Sum2 {
  double a, b;
};
__device__ inline Sum2 sum2_merge(const Sum2& x, const Sum2& y) { return {x.a + y.a, x.b + y.b}; }
__device__ inline void block_sum2(double& a, double& b) {
  const Sum2 r = block_reduce<SURF_THREADS, true>(Sum2{a, b}, sum2_merge);
  a = r.a;
  b = r.b;
}

// thread 0 has stored this workgroup's partials (store_agent); true in every thread of the workgroup that arrives last
__device__ inline bool arrive_last(unsigned* ticket, unsigned nblocks) {
  __shared__ unsigned last;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the partials have been acknowledged before the ticket is taken
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1u;
    if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
  }
  __syncthreads();
  return last != 0u;
}

// the last workgroup folds the two sums of every workgroup (fold_partials), read past the caches
__device__ inline void fold_sums(const double* part, unsigned nblocks, double& a, double& b) {
  const Sum2 r = fold_partials<SURF_THREADS, true>(nblocks, Sum2{0.0, 0.0}, [part](long k) { return Sum2{load_agent(part + 2 * k), load_agent(part + 2 * k + 1)}; },
                                             sum2_merge);
  a = r.a;
  b = r.b;
}

// diagonal of A at node (r, c): the squared coefficients of the differences that exist and contain the node
__device__ inline double surf_diag(long r, long c, long H, long W, double T) {
  const int bxx = (c >= 2) + 4 * (c >= 1 && c <= W - 2) + (c <= W - 3);
  const int byy = (r >= 2) + 4 * (r >= 1 && r <= H - 2) + (r <= H - 3);
  const int nc = (c >= 1) + (c <= W - 2), nr = (r >= 1) + (r <= H - 2);
  return (1.0 - T) * (double)(bxx + byy + 2 * nr * nc) + T * (double)(nr + nc);
}

// constraint nodes: their number and the lowest index (integer atomics only)
__global__ __launch_bounds__(SURF_THREADS) void surface_scan_kernel(const float* __restrict__ d, long n, SurfState* st) {
  unsigned cnt = 0, inv = 0;
  const long stride = (long)gridDim.x * SURF_THREADS;
  for (long i = (long)blockIdx.x * SURF_THREADS + threadIdx.x; i < n; i += stride) {
    const float v = d[i];
    if (v == v) {
      cnt += 1;
      const unsigned k = ~(unsigned)i;
      inv = k > inv ? k : inv;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
    const unsigned o = __shfl_down(inv, off, 64);
    inv = o > inv ? o : inv;
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(&st->constraints, cnt);
    atomicMax(&st->first_inv, inv);
  }
}

// mask = 1 on free nodes; v = d - m on constraint nodes, 0 on free nodes
__global__ __launch_bounds__(SURF_THREADS) void surface_setup_kernel(const float* __restrict__ d, long n, const SurfState* st,
                                                                      unsigned char* __restrict__ mask, double* __restrict__ v) {
  const double m = (double)d[~st->first_inv];
  const long stride = (long)gridDim.x * SURF_THREADS;
  for (long i = (long)blockIdx.x * SURF_THREADS + threadIdx.x; i < n; i += stride) {
    const float z = d[i];
    const bool free_node = !(z == z);
    mask[i] = free_node ? 1 : 0;
    v[i] = free_node ? 0.0 : (double)z - m;
  }
}

// iterate != 0: one conjugate-gradient step's A p (skipped when done, alpha formed by the last tile); 0: the right-hand side's A v
__global__ __launch_bounds__(SURF_THREADS) void surface_operator_kernel(const double* __restrict__ p, const unsigned char* __restrict__ mask,
                                                                         double* __restrict__ ap, long H, long W, double T, unsigned ntx,
                                                                         double* part, SurfState* st, int iterate) {
  if (iterate && st->done) return;
  __shared__ double s[SURF_LR][SURF_LC];
  const long r0 = (long)(blockIdx.x / ntx) * SURF_TR, c0 = (long)(blockIdx.x % ntx) * SURF_TC;
  for (int k = threadIdx.x; k < SURF_LR * SURF_LC; k += SURF_THREADS) {
    const int lr = k / SURF_LC, lc = k - lr * SURF_LC;
    const long r = r0 + lr - SURF_HALO, c = c0 + lc - SURF_HALO;
    s[lr][lc] = (r >= 0 && r < H && c >= 0 && c < W) ? p[r * W + c] : 0.0;
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long c = c0 + tx;
  const int lc = tx + SURF_HALO;
  double dot = 0.0, unused = 0.0;
#pragma unroll
  for (int q = 0; q < SURF_TR / 4; ++q) {
    const int lr = ty + 4 * q + SURF_HALO;
    const long r = r0 + ty + 4 * q;
    if (r >= H || c >= W) continue;
    const long i = r * W + c;
    if (!mask[i]) { ap[i] = 0.0; continue; }
#define U(dr, dc) s[lr + (dr)][lc + (dc)]
    const bool cl = c >= 1, cr = c <= W - 2, ru = r >= 1, rd = r <= H - 2;
    double b = 0.0, g = 0.0;
    // Dxx' Dxx, Dyy' Dyy: the second differences centred one node before, at and one node after this one
    if (c >= 2) b += U(0, -2) - 2.0 * U(0, -1) + U(0, 0);
    if (cl && cr) b -= 2.0 * (U(0, -1) - 2.0 * U(0, 0) + U(0, 1));
    if (c <= W - 3) b += U(0, 0) - 2.0 * U(0, 1) + U(0, 2);
    if (r >= 2) b += U(-2, 0) - 2.0 * U(-1, 0) + U(0, 0);
    if (ru && rd) b -= 2.0 * (U(-1, 0) - 2.0 * U(0, 0) + U(1, 0));
    if (r <= H - 3) b += U(0, 0) - 2.0 * U(1, 0) + U(2, 0);
    // 2 Dxy' Dxy: the four cells that have this node as a corner
    if (ru && cl) b += 2.0 * (U(0, 0) - U(0, -1) - U(-1, 0) + U(-1, -1));
    if (ru && cr) b -= 2.0 * (U(0, 1) - U(0, 0) - U(-1, 1) + U(-1, 0));
    if (rd && cl) b -= 2.0 * (U(1, 0) - U(1, -1) - U(0, 0) + U(0, -1));
    if (rd && cr) b += 2.0 * (U(1, 1) - U(1, 0) - U(0, 1) + U(0, 0));
    // Dx' Dx, Dy' Dy
    if (cl) g += U(0, 0) - U(0, -1);
    if (cr) g -= U(0, 1) - U(0, 0);
    if (ru) g += U(0, 0) - U(-1, 0);
    if (rd) g -= U(1, 0) - U(0, 0);
    const double v = (1.0 - T) * b + T * g;
    ap[i] = v;
    dot += U(0, 0) * v;
#undef U
  }
  if (!iterate) return;
  block_sum2(dot, unused);
  if (threadIdx.x == 0) {
    store_agent(part + 2 * (size_t)blockIdx.x, dot);
    store_agent(part + 2 * (size_t)blockIdx.x + 1, 0.0);
  }
  if (!arrive_last(&st->ticket[0], gridDim.x)) return;
  double pap, zero;
  fold_sums(part, gridDim.x, pap, zero);
  if (threadIdx.x == 0) {
    st->pap = pap;
    st->alpha = pap > 0.0 ? st->rz / pap : 0.0;
  }
}

// start != 0: r = b = -A v, z = r / diag, rz = r . z, bb = r . r (done at once when b = 0); 0: one step's x, r, z, rz, rr, beta
__global__ __launch_bounds__(SURF_THREADS) void surface_update_kernel(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                                       const double* __restrict__ ap, long H, long W, double T, double tol,
                                                                       double* part, SurfState* st, int start) {
  if (!start && st->done) return;
  const double alpha = start ? 0.0 : st->alpha;
  const long n = H * W, stride = (long)gridDim.x * SURF_THREADS;
  double rz = 0.0, rr = 0.0;
  for (long i = (long)blockIdx.x * SURF_THREADS + threadIdx.x; i < n; i += stride) {
    double ri;
    if (start) {
      ri = -ap[i];
    } else {
      x[i] += alpha * p[i];
      ri = r[i] - alpha * ap[i];
    }
    r[i] = ri;
    const long row = (long)((unsigned)i / (unsigned)W);   // (H W < 2^31: a 32-bit division)
    const double z = ri / surf_diag(row, i - row * W, H, W, T);
    rz += ri * z;
    rr += ri * ri;
  }
  block_sum2(rz, rr);
  if (threadIdx.x == 0) {
    store_agent(part + 2 * (size_t)blockIdx.x, rz);
    store_agent(part + 2 * (size_t)blockIdx.x + 1, rr);
  }
  if (!arrive_last(&st->ticket[1], gridDim.x)) return;
  fold_sums(part, gridDim.x, rz, rr);
  if (threadIdx.x != 0) return;
  if (start) {
    st->bb = rr;
    st->tol2bb = tol * tol * rr;
    st->beta = 0.0;
    st->done = rr > 0.0 ? 0 : 1;
  } else {
    st->beta = st->rz > 0.0 ? rz / st->rz : 0.0;
    st->iters += 1;
    if (!(rr > st->tol2bb)) st->done = 1;
  }
  st->rz = rz;
  st->rr = rr;
}

// start != 0: p = z; 0: p = z + beta p
__global__ __launch_bounds__(SURF_THREADS) void surface_direction_kernel(const double* __restrict__ r, double* __restrict__ p, long H, long W,
                                                                          double T, const SurfState* st, int start) {
  if (st->done) return;
  const double beta = st->beta;
  const long n = H * W, stride = (long)gridDim.x * SURF_THREADS;
  for (long i = (long)blockIdx.x * SURF_THREADS + threadIdx.x; i < n; i += stride) {
    const long row = (long)((unsigned)i / (unsigned)W);   // (H W < 2^31: a 32-bit division)
    const double z = r[i] / surf_diag(row, i - row * W, H, W, T);
    p[i] = start ? z : z + beta * p[i];
  }
}

// u = x + m on free nodes, d on constraint nodes; rounded to float32 once
__global__ __launch_bounds__(SURF_THREADS) void surface_finish_kernel(const float* __restrict__ d, const double* __restrict__ x,
                                                                       const unsigned char* __restrict__ mask, long n, const SurfState* st,
                                                                       float* __restrict__ out) {
  const double m = (double)d[~st->first_inv];
  const long stride = (long)gridDim.x * SURF_THREADS;
  for (long i = (long)blockIdx.x * SURF_THREADS + threadIdx.x; i < n; i += stride) out[i] = mask[i] ? (float)(x[i] + m) : d[i];
}

// grid[r, c] = NaN unless a non-NaN node (r', c') of data has (r - r')^2 + (c - c')^2 <= radius^2
__global__ __launch_bounds__(SURF_THREADS) void surface_mask_kernel(const float* __restrict__ data, float* __restrict__ grid, long H, long W,
                                                                     int radius) {
  const long n = H * W, stride = (long)gridDim.x * SURF_THREADS;
  const int r2 = radius * radius;
  for (long i = (long)blockIdx.x * SURF_THREADS + threadIdx.x; i < n; i += stride) {
    const long r = (long)((unsigned)i / (unsigned)W), c = i - r * W;
    bool keep = false;
    for (int dr = -radius; dr <= radius && !keep; ++dr) {
      const long rr = r + dr;
      if (rr < 0 || rr >= H) continue;
      for (int dc = -radius; dc <= radius; ++dc) {
        const long cc = c + dc;
        if (cc < 0 || cc >= W || dr * dr + dc * dc > r2) continue;
        const float v = data[rr * W + cc];
        if (v == v) { keep = true; break; }
      }
    }
    if (!keep) grid[i] = __builtin_nanf("");
  }
}

int flat_blocks(long n) { return grid_stride_blocks(n, SURF_THREADS, SURF_MAX_BLOCKS); }

}  // namespace

static long surface_tiles(long H, long W) { return ((H + SURF_TR - 1) / SURF_TR) * ((W + SURF_TC - 1) / SURF_TC); }

// the one layout of the workspace.  part: two sums per workgroup of whichever launch has more of them, the operator's tiles or the
// elementwise kernels' SURF_MAX_BLOCKS
size_t surface_layout(SurfaceArrays& v, long H, long W, Carver c) {
  const size_t n = (size_t)H * (size_t)W, tiles = (size_t)surface_tiles(H, W);
  v.state = c.take<SurfState>(1);
  v.part = c.take<double>(2 * (tiles > SURF_MAX_BLOCKS ? tiles : (size_t)SURF_MAX_BLOCKS));
  v.x = c.take<double>(n);
  v.r = c.take<double>(n);
  v.p = c.take<double>(n);
  v.ap = c.take<double>(n);
  v.mask = c.take<unsigned char>(n);
  return c.bytes();
}

size_t surface_workspace(long H, long W) { SurfaceArrays v; return surface_layout(v, H, W, Carver(nullptr)); }

bool surface_solve(const SurfaceLaunch& a, void* ws, hipStream_t s, double info[4]) {
  const long H = a.H, W = a.W, n = H * W;
  const long tiles = surface_tiles(H, W);
  const unsigned ntx = (unsigned)((W + SURF_TC - 1) / SURF_TC);
  SurfaceArrays v;
  surface_layout(v, H, W, Carver(ws));
  SurfState* st = (SurfState*)v.state;
  double *part = v.part, *x = v.x, *r = v.r, *p = v.p, *ap = v.ap;
  unsigned char* mask = v.mask;
  const int fb = flat_blocks(n);
  const dim3 blk(SURF_THREADS);
  SurfState host;

  DBM_HIP(hipMemsetAsync(st, 0, sizeof(SurfState), s));
  DBM_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), s));
  hipLaunchKernelGGL(surface_scan_kernel, dim3(fb), blk, 0, s, a.data, n, st);
  DBM_HIP(hipGetLastError());
  DBM_HIP(hipMemcpyAsync(&host, st, sizeof(SurfState), hipMemcpyDeviceToHost, s));
  DBM_HIP(hipStreamSynchronize(s));
  DBM_CHECK(host.constraints > 0, "dbm_grid_tension_surface: the raster has no constraint node (every node is NaN); nothing was written");

  hipLaunchKernelGGL(surface_setup_kernel, dim3(fb), blk, 0, s, a.data, n, st, mask, p);
  hipLaunchKernelGGL(surface_operator_kernel, dim3((unsigned)tiles), blk, 0, s, p, mask, ap, H, W, a.tension, ntx, part, st, 0);
  hipLaunchKernelGGL(surface_update_kernel, dim3(fb), blk, 0, s, x, r, p, ap, H, W, a.tension, a.tol, part, st, 1);
  hipLaunchKernelGGL(surface_direction_kernel, dim3(fb), blk, 0, s, r, p, H, W, a.tension, st, 1);
  DBM_HIP(hipGetLastError());
  int launched = 0;
  for (;;) {
    DBM_HIP(hipMemcpyAsync(&host, st, sizeof(SurfState), hipMemcpyDeviceToHost, s));
    DBM_HIP(hipStreamSynchronize(s));
    if (host.done || launched >= a.max_iter) break;
    const int batch = a.max_iter - launched < SURF_CHECK_EVERY ? a.max_iter - launched : SURF_CHECK_EVERY;
    for (int k = 0; k < batch; ++k) {
      hipLaunchKernelGGL(surface_operator_kernel, dim3((unsigned)tiles), blk, 0, s, p, mask, ap, H, W, a.tension, ntx, part, st, 1);
      hipLaunchKernelGGL(surface_update_kernel, dim3(fb), blk, 0, s, x, r, p, ap, H, W, a.tension, a.tol, part, st, 0);
      hipLaunchKernelGGL(surface_direction_kernel, dim3(fb), blk, 0, s, r, p, H, W, a.tension, st, 0);
    }
    DBM_HIP(hipGetLastError());
    launched += batch;
  }
  hipLaunchKernelGGL(surface_finish_kernel, dim3(fb), blk, 0, s, a.data, x, mask, n, st, a.out);
  DBM_HIP(hipGetLastError());
  DBM_HIP(hipStreamSynchronize(s));
  info[0] = (double)host.iters;
  info[1] = host.bb > 0.0 ? std::sqrt(host.rr / host.bb) : 0.0;
  info[2] = (double)host.constraints;
  info[3] = (double)(n - (long)host.constraints);
  return host.done != 0;
}

void launch_distance_mask(const float* data, float* grid, long H, long W, int radius, hipStream_t s) {
  hipLaunchKernelGGL(surface_mask_kernel, dim3(flat_blocks(H * W)), dim3(SURF_THREADS), 0, s, data, grid, H, W, radius);
  DBM_HIP(hipGetLastError());
}

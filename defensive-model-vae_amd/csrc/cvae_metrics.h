// cvae_metrics.h — the count/sum tables of the model-vs-human validation (Distribution.py :195-331,
// Spatial_Distribution.py :18-161, :387-492, :708-931, :1357-1429) for a ragged population of
// trajectories: rows [n_rows][stride] float64, trajectory p owning rows [off[p], off[p+1]).
//
// Two passes.  val_ranges_kernel reduces min/max of v, x, y, t (exact, order-independent) so the
// HOST can build every bin edge with numpy exactly as the reference does; val_accumulate_kernel
// then binary-searches those edge VALUES (never floor((x-x0)/h)), which is what makes the integer
// tables bit-equal to np.histogram / np.histogram2d / np.digitize.  One wavefront per trajectory,
// lanes striding over its points (the MPC kernel's convention).
//
// Determinism: every table is an integer.  Floating sums are 64-bit fixed point, quantum 2^-24,
// each addend rounded to nearest (|value| < 1024 and < 2^28 points are checked on the host, so
// |sum| < 2^62): integer addition is associative, so the tables do not depend on the launch
// geometry or the order of the atomics.  No f64 atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VAL_MAX_EDGES 1024     // per axis
#define VAL_MAX_CELLS 65536    // scene grid cells (8 KB of visited-mask per wave)
#define VAL_MAX_SLICES 4096    // M5 time slices
#define VAL_MAX_SURF 4096      // M4 surface cells
#define VAL_LDS_SLICES 256     // slices privatised in LDS; more go straight to global atomics
#define VAL_MAX_WAVES 8
#define VAL_FIX_SCALE 16777216.0  // 2^24

struct ValCfg {
  double dt;
  int stride, x_col, y_col, t_col, v_col, coord_col, subsample, surf_min_rows;
  int n_v, n_x, n_y, n_c, n_t, n_s;  // edge counts (0 = that table is off)
};

struct ValTables {
  unsigned int* hist_v;       // [n_v-1]
  unsigned int* h_points;     // [n_y-1][n_x-1]
  unsigned int* h_traj;       // [n_y-1][n_x-1]
  unsigned int* surf_cnt;     // [n_t-1][n_c-1]
  long long* surf_sum;        // [n_t-1][n_c-1], fixed point
  unsigned int* slice_cnt;    // [n_s-1]
  long long* slice_sx;        // [n_s-1], fixed point
  long long* slice_sy;        // [n_s-1], fixed point
};

// ranges output, 16 x 64-bit words: keys (val_key) of min/max of v, x, y, t over every point
// [0..7], of x, y, t over the trajectories with >= surf_min_rows rows [8..13], the point count
// [14] and the longest trajectory [15].
enum { VAL_R_V = 0, VAL_R_X = 2, VAL_R_Y = 4, VAL_R_T = 6, VAL_R_SX = 8, VAL_R_SY = 10, VAL_R_ST = 12,
       VAL_R_COUNT = 14, VAL_R_LONGEST = 15, VAL_R_WORDS = 16 };

// order-preserving map double -> u64 (so integer atomicMin/atomicMax reduce doubles exactly)
__device__ __forceinline__ unsigned long long val_key(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void val_ranges_init_kernel(unsigned long long* out) {
  const int i = threadIdx.x;
  if (i < VAL_R_COUNT) out[i] = (i & 1) ? 0ull : ~0ull;  // max slots start at the lowest key, min at the highest
  else if (i < VAL_R_WORDS) out[i] = 0ull;
}

__device__ __forceinline__ unsigned long long val_wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long val_wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// model time of point i: np.arange(n) * dt (Spatial_Distribution.py:733, :1393) — one rounded product
__device__ __forceinline__ double val_time(const ValCfg& c, const double* r, int64_t i) {
  return c.t_col >= 0 ? r[c.t_col] : __dmul_rn((double)i, c.dt);
}

__global__ void val_ranges_kernel(ValCfg c, int n_traj, const double* __restrict__ rows,
                                  const int64_t* __restrict__ off, int64_t n_rows, const double* __restrict__ v_arr,
                                  unsigned long long* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  unsigned long long mn[4] = {~0ull, ~0ull, ~0ull, ~0ull}, mx[4] = {0, 0, 0, 0};
  unsigned long long smn[3] = {~0ull, ~0ull, ~0ull}, smx[3] = {0, 0, 0};
  unsigned long long count = 0, longest = 0;
  for (int64_t p = (int64_t)blockIdx.x * waves + wave; p < n_traj; p += (int64_t)gridDim.x * waves) {
    int64_t b = off[p], e = off[p + 1];
    b = b < 0 ? 0 : b;
    e = e > n_rows ? n_rows : e;  // host-validated; clipped all the same
    const int64_t n = e - b;
    if (n <= 0) continue;
    const bool surf = n >= c.surf_min_rows;
    for (int64_t i = lane; i < n; i += 64) {
      const double* r = rows + (b + i) * c.stride;
      const double q[4] = {c.v_col >= 0 ? r[c.v_col] : v_arr[b + i], r[c.x_col], r[c.y_col], val_time(c, r, i)};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (q[k] != q[k]) continue;  // NaN: a row without a value (the v of a one-point human track)
        const unsigned long long key = val_key(q[k]);
        mn[k] = key < mn[k] ? key : mn[k];
        mx[k] = key > mx[k] ? key : mx[k];
        if (k > 0 && surf) {
          smn[k - 1] = key < smn[k - 1] ? key : smn[k - 1];
          smx[k - 1] = key > smx[k - 1] ? key : smx[k - 1];
        }
      }
    }
    if (lane == 0) {
      count += (unsigned long long)n;
      longest = (unsigned long long)n > longest ? (unsigned long long)n : longest;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long a = val_wave_min(mn[k]), z = val_wave_max(mx[k]);
    if (lane == 0 && a <= z) {  // a > z: this wave saw no point
      atomicMin(&out[2 * k], a);
      atomicMax(&out[2 * k + 1], z);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned long long a = val_wave_min(smn[k]), z = val_wave_max(smx[k]);
    if (lane == 0 && a <= z) {
      atomicMin(&out[VAL_R_SX + 2 * k], a);
      atomicMax(&out[VAL_R_SX + 2 * k + 1], z);
    }
  }
  if (lane == 0 && count) {
    atomicAdd(&out[VAL_R_COUNT], count);
    atomicMax(&out[VAL_R_LONGEST], longest);
  }
}

// number of edges <= x (np.digitize(x, edges) for increasing edges, np.searchsorted side='right')
__device__ __forceinline__ int val_upper(const double* e, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// np.digitize(x, edges) - 1 clipped to the grid (Spatial_Distribution.py:415-420, :906-910)
__device__ __forceinline__ int val_clip_bin(const double* e, int n, double x) {
  int i = val_upper(e, n, x) - 1;
  i = i < 0 ? 0 : i;
  return i > n - 2 ? n - 2 : i;
}
// np.histogram / np.histogramdd with explicit edges: outside [first, last] dropped (-1), last bin closed
__device__ __forceinline__ int val_hist_bin(const double* e, int n, double x) {
  if (!(x >= e[0]) || !(x <= e[n - 1])) return -1;
  const int i = val_upper(e, n, x) - 1;
  return i > n - 2 ? n - 2 : i;
}
// addend of the fixed-point sums: round-to-nearest multiple of 2^-24, saturated at the host-checked bound
__device__ __forceinline__ long long val_fix(double v) {
  v = v > 1024.0 ? 1024.0 : (v < -1024.0 ? -1024.0 : v);
  return v == v ? __double2ll_rn(v * VAL_FIX_SCALE) : 0ll;
}

// LDS bytes of one workgroup (host and device agree through this one function)
__host__ __device__ inline size_t val_lds_bytes(const ValCfg& c, int waves) {
  const int n_staged_s = (c.n_s >= 2 && c.n_s - 1 <= VAL_LDS_SLICES) ? c.n_s : 0;
  const int ls = n_staged_s ? c.n_s - 1 : 0;
  const int surf = (c.n_c >= 2 && c.n_t >= 2) ? (c.n_c - 1) * (c.n_t - 1) : 0;
  const int cells = (c.n_x >= 2 && c.n_y >= 2) ? (c.n_x - 1) * (c.n_y - 1) : 0;
  const int words = (cells + 31) / 32;
  size_t b = (size_t)(c.n_v + c.n_x + c.n_y + c.n_c + c.n_t + n_staged_s) * 8;  // edges
  b += (size_t)(surf + 2 * ls) * 8;                                              // surf_sum, slice sx/sy
  b += (size_t)(surf + ls + (c.n_v >= 2 ? c.n_v - 1 : 0)) * 4;                   // surf_cnt, slice_cnt, hist_v
  b += (size_t)words * waves * 4;                                                // visited masks
  return (b + 7) / 8 * 8;
}

// edges: the six edge arrays back to back in the order v, x, y, coordinate, time, slice.
__global__ void val_accumulate_kernel(ValCfg c, int n_traj, const double* __restrict__ rows,
                                      const int64_t* __restrict__ off, int64_t n_rows,
                                      const double* __restrict__ v_hist, const double* __restrict__ v_surf,
                                      const double* __restrict__ edges, ValTables T) {
  extern __shared__ double val_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const bool on_v = c.n_v >= 2, on_grid = c.n_x >= 2 && c.n_y >= 2, on_surf = c.n_c >= 2 && c.n_t >= 2;
  const bool on_s = c.n_s >= 2;
  const int ns = on_s ? c.n_s - 1 : 0;
  const bool lds_s = on_s && ns <= VAL_LDS_SLICES;
  const int ls = lds_s ? ns : 0;
  const int surf = on_surf ? (c.n_c - 1) * (c.n_t - 1) : 0;
  const int gx = on_grid ? c.n_x - 1 : 0, cells = on_grid ? gx * (c.n_y - 1) : 0, words = (cells + 31) / 32;
  const int nbins = on_v ? c.n_v - 1 : 0;
  const int n_edges = c.n_v + c.n_x + c.n_y + c.n_c + c.n_t + (lds_s ? c.n_s : 0);

  double* ev = val_lds;
  double* ex = ev + c.n_v;
  double* ey = ex + c.n_x;
  double* ec = ey + c.n_y;
  double* et = ec + c.n_c;
  const double* es = lds_s ? et + c.n_t : edges + (c.n_v + c.n_x + c.n_y + c.n_c + c.n_t);
  long long* l_ssum = (long long*)(val_lds + n_edges);
  long long* l_sx = l_ssum + surf;
  long long* l_sy = l_sx + ls;
  unsigned int* l_scnt = (unsigned int*)(l_sy + ls);
  unsigned int* l_slc = l_scnt + surf;
  unsigned int* l_hist = l_slc + ls;
  unsigned int* l_mask = l_hist + nbins + (size_t)wave * words;

  for (int i = tid; i < n_edges; i += blockDim.x) val_lds[i] = edges[i];
  {
    unsigned int* z = (unsigned int*)(val_lds + n_edges);
    const int nz = 2 * (surf + 2 * ls) + surf + ls + nbins + words * waves;
    for (int i = tid; i < nz; i += blockDim.x) z[i] = 0u;
  }
  __syncthreads();

  for (int64_t p = (int64_t)blockIdx.x * waves + wave; p < n_traj; p += (int64_t)gridDim.x * waves) {
    int64_t b = off[p], e = off[p + 1];
    b = b < 0 ? 0 : b;
    e = e > n_rows ? n_rows : e;
    const int64_t n = e - b;
    if (n <= 0) continue;
    const bool surf_on = on_surf && n >= c.surf_min_rows;
    for (int64_t i = lane; i < n; i += 64) {
      const double* r = rows + (b + i) * c.stride;
      const double x = r[c.x_col], y = r[c.y_col];
      const double t = val_time(c, r, i);
      if (on_v) {  // M1
        const int k = val_hist_bin(ev, c.n_v, c.v_col >= 0 ? r[c.v_col] : v_hist[b + i]);
        if (k >= 0) atomicAdd(&l_hist[k], 1u);
      }
      if (on_grid && x == x && y == y) {  // M3: border cells take what lies outside
        const int cell = val_clip_bin(ey, c.n_y, y) * gx + val_clip_bin(ex, c.n_x, x);
        atomicOr(&l_mask[cell >> 5], 1u << (cell & 31));
      }
      if (surf_on) {  // M4
        const double cc = r[c.coord_col];
        if (cc == cc && t == t) {
          const int cell = val_clip_bin(et, c.n_t, t) * (c.n_c - 1) + val_clip_bin(ec, c.n_c, cc);
          atomicAdd(&l_scnt[cell], 1u);
          atomicAdd((unsigned long long*)&l_ssum[cell],
                    (unsigned long long)val_fix(c.v_col >= 0 ? r[c.v_col] : v_surf[b + i]));
        }
      }
      if (on_s) {  // M5: half-open slices
        const int k = val_upper(es, c.n_s, t) - 1;
        if (k >= 0 && k < ns && x == x && y == y) {
          const unsigned long long fx = (unsigned long long)val_fix(x), fy = (unsigned long long)val_fix(y);
          if (lds_s) {
            atomicAdd(&l_slc[k], 1u);
            atomicAdd((unsigned long long*)&l_sx[k], fx);
            atomicAdd((unsigned long long*)&l_sy[k], fy);
          } else {
            atomicAdd(&T.slice_cnt[k], 1u);
            atomicAdd((unsigned long long*)&T.slice_sx[k], fx);
            atomicAdd((unsigned long long*)&T.slice_sy[k], fy);
          }
        }
      }
    }
    if (on_grid) {
      // M2: every point if n <= subsample, else np.linspace(0, n-1, subsample, dtype=int):
      // floor(k * ((n-1)/(subsample-1))), the last index set to n-1 (numpy's linspace, restated)
      const bool sub = c.subsample > 1 && n > c.subsample;
      const int64_t m = sub ? c.subsample : n;
      const double step = sub ? __ddiv_rn((double)(n - 1), (double)(c.subsample - 1)) : 1.0;
      for (int64_t k = lane; k < m; k += 64) {
        int64_t i = sub ? (k == m - 1 ? n - 1 : (int64_t)floor(__dmul_rn((double)k, step))) : k;
        i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
        const double* r = rows + (b + i) * c.stride;
        const int ix = val_hist_bin(ex, c.n_x, r[c.x_col]), iy = val_hist_bin(ey, c.n_y, r[c.y_col]);
        if (ix >= 0 && iy >= 0) atomicAdd(&T.h_points[iy * gx + ix], 1u);
      }
      // sweep this wave's visited mask: +1 per cell per trajectory, and clear it for the next one.
      // The mask belongs to this wave alone and a wave's LDS operations complete in order.
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int w = lane; w < words; w += 64) {
        unsigned int mword = l_mask[w];
        l_mask[w] = 0u;
        while (mword) {
          const int bit = __ffs(mword) - 1;
          mword &= mword - 1;
          const int cell = w * 32 + bit;
          if (cell < cells) atomicAdd(&T.h_traj[cell], 1u);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
  __syncthreads();
  for (int i = tid; i < nbins; i += blockDim.x)
    if (l_hist[i]) atomicAdd(&T.hist_v[i], l_hist[i]);
  for (int i = tid; i < surf; i += blockDim.x)
    if (l_scnt[i]) {
      atomicAdd(&T.surf_cnt[i], l_scnt[i]);
      atomicAdd((unsigned long long*)&T.surf_sum[i], (unsigned long long)l_ssum[i]);
    }
  for (int i = tid; i < ls; i += blockDim.x)
    if (l_slc[i]) {
      atomicAdd(&T.slice_cnt[i], l_slc[i]);
      atomicAdd((unsigned long long*)&T.slice_sx[i], (unsigned long long)l_sx[i]);
      atomicAdd((unsigned long long*)&T.slice_sy[i], (unsigned long long)l_sy[i]);
    }
}

// cvae_safety.h — the SUT_Testing stage for a whole population of tracked trajectories: the
// write-back of a track [x, y, theta, v] into the human log it started from (Defensive_Testing.py
// find_best_start_row :156-163, compute_ego_kinematics :130-153, merge_trajectory_into_csv :166-205)
// and the safety metrics of the merged log (tools/Metrics_Calculation.py: the four scenario filters
// :143-210, add_ttc_column :264-274, _pet_two_rays :19-63, add_jerk_column :300-328 and the
// scenario sub-window statistics of main() :412-456 with metric = "TTC").
//
// Logs: [SF_NCOL][n_rows] float64, column-major, log f owning rows [off[f], off[f+1]); read-only,
// many tracks may share one.  Tracks: the ragged layout cvae_mpc_track writes, rows [n][4].
// One wavefront per track, lanes striding over rows (cvae_mpc.h / cvae_metrics.h convention),
// workgroups looping over tracks.  The merged log is never written: sf_chunk_ego returns the merged
// ego state of a row, staging the neighbours' vx, vy of a 64-row chunk in LDS (one-row halo) for
// np.gradient.
//
// Numerics: plain float64, every value-producing function with contraction off, so each numpy
// operation is one rounded operation here.  Per-track sums: lane-strided partials in row order,
// then a fixed xor butterfly — bit-identical from run to run and whatever the waves per workgroup.
// No floating atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

enum { SF_FRAME = 0, SF_TIME, SF_EGO_X, SF_EGO_Y, SF_EGO_VX, SF_EGO_VY, SF_EGO_AX, SF_EGO_AY, SF_EGO_YAW,
       SF_SV1_X, SF_SV1_Y, SF_SV1_VX, SF_SV1_VY, SF_SV1_AX, SF_SV1_YAW,
       SF_SV2_X, SF_SV2_Y, SF_SV2_VX, SF_SV2_VY, SF_SV2_YAW, SF_NCOL };
// scene ids: cvae_scene (include/cvae.h)
enum { SF_STATIC = 0, SF_DYNAMIC = 1, SF_PREDICTABLE = 2, SF_UNPREDICTABLE = 3 };
enum { SF_OK = 0, SF_NO_WINDOW = 1, SF_EMPTY = 2, SF_NO_START = 3 };
// per-track record (float64 words; the integer fields are exact)
enum { SF_R_STATUS = 0, SF_R_START, SF_R_L, SF_R_I0, SF_R_I1, SF_R_NWIN, SF_R_NSUB,
       SF_R_TTC_N, SF_R_TTC_MEAN, SF_R_TTC_MIN, SF_R_PET_N, SF_R_PET_MEAN, SF_R_PET_MIN,
       SF_R_JERK_N, SF_R_JERK_MEAN, SF_R_JERK_MAX, SF_R_DECEL, SF_R_YAW_MAX, SF_REC };
// per-row output columns
enum { SF_O_TTC = 0, SF_O_PET, SF_O_JERK, SF_O_EGO, SF_O_NCOL = SF_O_EGO + 7 };
enum { SF_E_X = 0, SF_E_Y, SF_E_VX, SF_E_VY, SF_E_AX, SF_E_AY, SF_E_YAW };
enum { SF_ROWS_WINDOW = 1, SF_ROWS_EGO = 2 };
#define SF_MAX_WAVES 8
#define SF_LDS_ROW 66  // 64 rows + one halo row on each side

// The scenario table (Metrics_Calculation.py; mirrored by cvae_amd.safety.SCENARIOS, which the numpy
// oracle uses — tests/test_safety_oracle.py checks the two against each other).
#define SF_EPS_V 1e-9          // EPS_V :15
#define SF_EPS_DET 1e-12       // EPS_DET :16
#define SF_DT_STATIC 0.02      // _default_dt_jerk :289-297
#define SF_DT_DYNAMIC 0.025
#define SF_DT_PREDICTABLE 0.015
#define SF_DT_UNPREDICTABLE 0.02
#define SF_STATIC_END_Y 80.0            // :150
#define SF_DYNAMIC_START_YAW -150.0     // :159
#define SF_DYNAMIC_END_X -186.8897      // :164
#define SF_PREDICTABLE_START_Y 40.0     // :175
#define SF_PREDICTABLE_END_Y -78.0      // :184
#define SF_UNPRED_DIST 30.0             // :198
#define SF_UNPRED_AX 0.1                // :198, :206
#define SF_UNPRED_END_YAW -90.0         // :206
#define SF_UNPRED_END_X 15.0            // :206
#define SF_SUB_STATIC_LO -196.81        // main() :413
#define SF_SUB_STATIC_HI -193.31
#define SF_SUB_DYNAMIC_AX 100.0         // :422
#define SF_SUB_PREDICTABLE_X 156.76     // :436
#define SF_SUB_LANE_X1 13.06            // :444-445
#define SF_SUB_LANE_Y1 -160.0
#define SF_SUB_LANE_X2 14.77
#define SF_SUB_LANE_Y2 220.0

struct SfArgs {
  const double* cols;        // [SF_NCOL][n_log_rows]
  const int64_t* log_off;    // [n_logs + 1]
  const int32_t* log_flags;  // [n_logs], bit 0: the log has sim_time
  const double* states;      // [n_state_rows][4], or null when merge == 0
  const int64_t* off;        // [P + 1]
  const int32_t* log_of_track;  // [P]
  double* records;           // [P][SF_REC]
  double* rows;              // [SF_O_NCOL][n_out_rows], or null
  const int64_t* row_off;    // [P + 1]: track p owns out rows [row_off[p], row_off[p+1])
  int64_t n_log_rows, n_state_rows, n_out_rows;
  int n_logs, P, scene, want_rows, merge;
};

// one track's view of its log and its states (wave-uniform)
struct SfTrack {
  const double* cols;   // column 0 of the log's first row
  int64_t stride;       // rows per column
  const double* st;     // the track's first state row
  int64_t n_log, start, L, M;  // merged row r: the log's for r < start, the track's for start <= r < M = start + L
  double dx0;           // frame[start + 1] - frame[start]
  int scene;
  bool uniform;         // np.gradient's uniform-spacing case: every frame difference == dx0
  bool has_time;
};

__device__ __forceinline__ double sf_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double sf_col(const SfTrack& T, int c, int64_t r) { return T.cols[c * T.stride + r]; }

__device__ __forceinline__ double sf_default_dt(int scene) {
  switch (scene) {
    case SF_STATIC: return SF_DT_STATIC;
    case SF_DYNAMIC: return SF_DT_DYNAMIC;
    case SF_PREDICTABLE: return SF_DT_PREDICTABLE;
    default: return SF_DT_UNPREDICTABLE;
  }
}

// merged ego position of row r (0 <= r < M)
__device__ __forceinline__ void sf_ego_xy(const SfTrack& T, int64_t r, double& x, double& y) {
  if (r < T.start) {
    x = sf_col(T, SF_EGO_X, r);
    y = sf_col(T, SF_EGO_Y, r);
  } else {
    const double* s = T.st + (r - T.start) * 4;
    x = s[0];
    y = s[1];
  }
}

// merged ego velocity of row r: vx = v*cos(theta), vy = v*sin(theta) on the track (:143-144); rows
// outside the merged log give 0 (they are staged but never used)
__device__ __forceinline__ void sf_ego_v(const SfTrack& T, int64_t r, double& vx, double& vy) {
#pragma clang fp contract(off)
  vx = vy = 0.0;
  if (r < 0 || r >= T.M) return;
  if (r < T.start) {
    vx = sf_col(T, SF_EGO_VX, r);
    vy = sf_col(T, SF_EGO_VY, r);
  } else {
    const double* s = T.st + (r - T.start) * 4;
    vx = s[3] * cos(s[2]);
    vy = s[3] * sin(s[2]);
  }
}

// np.gradient(f, t)[k] for a segment of L samples (numpy/lib/function_base.py gradient, edge_order 1):
// first-order one-sided edges; inside, (f[k+1] - f[k-1]) / (2 dx) when the spacing is uniform, else
// the second-order formula with hd = t[k] - t[k-1], hs = t[k+1] - t[k].  L == 1 gives 0 (:147-149).
__device__ __forceinline__ double sf_gradient(double fm, double f0, double fp, double tm, double t0, double tp,
                                              int64_t k, int64_t L, bool uniform, double dx0) {
#pragma clang fp contract(off)
  if (L == 1) return 0.0;
  if (k == 0) return (fp - f0) / (uniform ? dx0 : tp - t0);
  if (k == L - 1) return (f0 - fm) / (uniform ? dx0 : t0 - tm);
  if (uniform) return (fp - fm) / (2.0 * dx0);
  const double hd = t0 - tm, hs = tp - t0;
  const double a = -(hs) / (hd * (hd + hs));
  const double b = (hs - hd) / (hd * hs);
  const double c = hd / (hs * (hd + hs));
  return a * fm + b * f0 + c * fp;
}

// Merged ego state (x, y, vx, vy, ax, ay, yaw) of row base + lane.  Wave-wide: every lane calls it;
// the chunk's vx, vy go to this wave's LDS rows (slot lane + 1; lanes 0 and 1 also stage the halo
// rows base - 1 and base + 64), so a row's cos/sin are evaluated once, not once per neighbour.
__device__ __forceinline__ void sf_chunk_ego(const SfTrack& T, int64_t base, int lane, double* lvx, double* lvy,
                                             double ego[7]) {
#pragma clang fp contract(off)
  const int64_t r = base + lane;
  double vx, vy;
  sf_ego_v(T, r, vx, vy);
  lvx[lane + 1] = vx;
  lvy[lane + 1] = vy;
  if (lane < 2) {
    double hx, hy;
    sf_ego_v(T, lane == 0 ? base - 1 : base + 64, hx, hy);
    lvx[lane == 0 ? 0 : 65] = hx;
    lvy[lane == 0 ? 0 : 65] = hy;
  }
  // the rows belong to this wave alone and a wave's LDS operations complete in order
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const double nan = sf_nan();
  for (int k = 0; k < 7; ++k) ego[k] = nan;
  if (r >= 0 && r < T.M) {
    if (r < T.start) {
      ego[SF_E_X] = sf_col(T, SF_EGO_X, r);
      ego[SF_E_Y] = sf_col(T, SF_EGO_Y, r);
      ego[SF_E_VX] = vx;
      ego[SF_E_VY] = vy;
      ego[SF_E_AX] = sf_col(T, SF_EGO_AX, r);
      ego[SF_E_AY] = sf_col(T, SF_EGO_AY, r);
      ego[SF_E_YAW] = sf_col(T, SF_EGO_YAW, r);
    } else {
      const int64_t k = r - T.start;
      const double* s = T.st + k * 4;
      const double t0 = sf_col(T, SF_FRAME, r);
      const double tm = k > 0 ? sf_col(T, SF_FRAME, r - 1) : t0;
      const double tp = k < T.L - 1 ? sf_col(T, SF_FRAME, r + 1) : t0;
      ego[SF_E_X] = s[0];
      ego[SF_E_Y] = s[1];
      ego[SF_E_VX] = vx;
      ego[SF_E_VY] = vy;
      ego[SF_E_AX] = sf_gradient(lvx[lane], vx, lvx[lane + 2], tm, t0, tp, k, T.L, T.uniform, T.dx0);
      ego[SF_E_AY] = sf_gradient(lvy[lane], vy, lvy[lane + 2], tm, t0, tp, k, T.L, T.uniform, T.dx0);
      ego[SF_E_YAW] = s[2] * (180.0 / M_PI);  // np.rad2deg (:145)
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the scenario's start predicate on merged row r (filter_* :145, :159, :174-179, :193-198)
__device__ __forceinline__ bool sf_start_pred(const SfTrack& T, int64_t r) {
#pragma clang fp contract(off)
  double ex, ey;
  sf_ego_xy(T, r, ex, ey);
  switch (T.scene) {
    case SF_STATIC:
      return ey > 0.0 && sf_col(T, SF_SV2_VX, r) != 0.0 && sf_col(T, SF_SV2_VY, r) != 0.0;
    case SF_DYNAMIC:
      return sf_col(T, SF_SV1_YAW, r) < SF_DYNAMIC_START_YAW;
    case SF_PREDICTABLE:
      return ey < SF_PREDICTABLE_START_Y && ey != 0.0 && sf_col(T, SF_SV1_VX, r) != 0.0 &&
             sf_col(T, SF_SV1_VY, r) != 0.0;
    default: {
      const double dx = ex - sf_col(T, SF_SV1_X, r), dy = ey - sf_col(T, SF_SV1_Y, r);
      return sqrt(dx * dx + dy * dy) <= SF_UNPRED_DIST && fabs(sf_col(T, SF_SV1_AX, r)) >= SF_UNPRED_AX;
    }
  }
}

// the scenario's end predicate (:150, :164, :184, :206)
__device__ __forceinline__ bool sf_end_pred(const SfTrack& T, int64_t r) {
  double ex, ey;
  sf_ego_xy(T, r, ex, ey);
  switch (T.scene) {
    case SF_STATIC: return ey >= SF_STATIC_END_Y;
    case SF_DYNAMIC: return ex < SF_DYNAMIC_END_X;
    case SF_PREDICTABLE: return ey < SF_PREDICTABLE_END_Y;
    default: {
      const double ax = sf_col(T, SF_SV1_AX, r);
      return fabs(ax) < SF_UNPRED_AX && sf_col(T, SF_SV1_YAW, r) < SF_UNPRED_END_YAW && ax != 0.0 &&
             sf_col(T, SF_SV1_X, r) > SF_UNPRED_END_X;
    }
  }
}

// first row in [from, to) meeting a predicate, -1 if none: 64-row ballots, early exit
template <bool END>
__device__ __forceinline__ int64_t sf_first(const SfTrack& T, int64_t from, int64_t to, int lane) {
  for (int64_t base = from; base < to; base += 64) {
    const int64_t r = base + lane;
    const bool hit = r < to && (END ? sf_end_pred(T, r) : sf_start_pred(T, r));
    const unsigned long long m = __ballot(hit);
    if (m) return base + (__ffsll((long long)m) - 1);
  }
  return -1;
}

// one-dimensional TTC along the scenario's axis against its vehicle (add_ttc_column :264-274,
// ttc_axis_* :213-249): num / denom, NaN where |denom| <= EPS_V
__device__ __forceinline__ double sf_ttc(const SfTrack& T, int64_t r, const double ego[7]) {
#pragma clang fp contract(off)
  double num, denom;
  switch (T.scene) {
    case SF_STATIC:
      num = sf_col(T, SF_SV2_Y, r) - ego[SF_E_Y];
      denom = ego[SF_E_VY] - sf_col(T, SF_SV2_VY, r);
      break;
    case SF_DYNAMIC:
      num = sf_col(T, SF_SV2_X, r) - ego[SF_E_X];
      denom = ego[SF_E_VX] - sf_col(T, SF_SV2_VX, r);
      break;
    default:
      num = sf_col(T, SF_SV1_Y, r) - ego[SF_E_Y];
      denom = ego[SF_E_VY] - sf_col(T, SF_SV1_VY, r);
  }
  return fabs(denom) > SF_EPS_V ? num / denom : sf_nan();
}

// _pet_two_rays (:19-63) of the ego against sv2 (Static, Dynamic) or sv1 (add_pet_column :277-286)
__device__ __forceinline__ double sf_pet(const SfTrack& T, int64_t r, const double ego[7]) {
#pragma clang fp contract(off)
  const bool two = T.scene == SF_STATIC || T.scene == SF_DYNAMIC;
  const double px2 = sf_col(T, two ? SF_SV2_X : SF_SV1_X, r), py2 = sf_col(T, two ? SF_SV2_Y : SF_SV1_Y, r);
  const double vx2 = sf_col(T, two ? SF_SV2_VX : SF_SV1_VX, r), vy2 = sf_col(T, two ? SF_SV2_VY : SF_SV1_VY, r);
  const double yaw2 = sf_col(T, two ? SF_SV2_YAW : SF_SV1_YAW, r);
  const double sp1 = hypot(ego[SF_E_VX], ego[SF_E_VY]), sp2 = hypot(vx2, vy2);
  const double th1 = ego[SF_E_YAW] * (M_PI / 180.0), th2 = yaw2 * (M_PI / 180.0);  // np.deg2rad
  const double V1x = sp1 * cos(th1), V1y = sp1 * sin(th1);
  const double V2x = sp2 * cos(th2), V2y = sp2 * sin(th2);
  const double dpx = px2 - ego[SF_E_X], dpy = py2 - ego[SF_E_Y];
  const double det = V1x * (-V2y) - (-V2x) * V1y;
  const double t1 = (dpx * (-V2y) - dpy * (-V2x)) / det;
  const double t2 = (V1x * dpy - V1y * dpx) / det;
  const bool invalid = fabs(det) < SF_EPS_DET || sp1 < SF_EPS_V || sp2 < SF_EPS_V || t1 < 0.0 || t2 < 0.0 ||
                       !isfinite(t1) || !isfinite(t2);
  return invalid ? sf_nan() : fabs(t1 - t2);
}

__device__ __forceinline__ double sf_wave_sum(double v) {
#pragma clang fp contract(off)
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double sf_wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ double sf_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ void sf_write_record(double* rec, int lane, int status, int64_t start, int64_t L) {
  if (lane < SF_REC) rec[lane] = lane == SF_R_STATUS ? (double)status
                                 : lane == SF_R_START ? (double)start
                                 : lane == SF_R_L ? (double)L
                                 : (lane == SF_R_I0 || lane == SF_R_I1) ? -1.0
                                 : (lane == SF_R_NWIN || lane == SF_R_NSUB || lane == SF_R_TTC_N ||
                                    lane == SF_R_PET_N || lane == SF_R_JERK_N) ? 0.0 : sf_nan();
}

__device__ void sf_track(const SfArgs& A, int64_t p, int lane, double* lvx, double* lvy) {
#pragma clang fp contract(off)
  double* rec = A.records + p * SF_REC;
  const int lg = A.log_of_track[p];
  int64_t b = 0, e = 0;
  if (lg >= 0 && lg < A.n_logs) {  // host-validated; clipped all the same
    b = A.log_off[lg];
    e = A.log_off[lg + 1];
    b = b < 0 ? 0 : b;
    e = e > A.n_log_rows ? A.n_log_rows : e;
  }
  SfTrack T;
  T.cols = A.cols + b;
  T.stride = A.n_log_rows;
  T.n_log = e > b ? e - b : 0;
  T.scene = A.scene;
  T.has_time = T.n_log > 0 && (A.log_flags[lg] & 1);
  T.st = nullptr;
  T.uniform = true;
  T.dx0 = 0.0;
  int64_t n_track = 0;
  if (A.merge) {
    int64_t tb = A.off[p], te = A.off[p + 1];
    tb = tb < 0 ? 0 : tb;
    te = te > A.n_state_rows ? A.n_state_rows : te;
    n_track = te > tb ? te - tb : 0;
    T.st = A.states + tb * 4;
  }
  if (T.n_log == 0 || (A.merge && n_track == 0)) {
    sf_write_record(rec, lane, SF_EMPTY, -1, 0);
    return;
  }

  if (A.merge) {
    // 1. start = np.nanargmin((ego_x - x0)^2 + (ego_y - y0)^2): lane-strided, then a butterfly on
    //    (value, index); the lowest index wins ties (:156-163)
    const double x0 = T.st[0], y0 = T.st[1];
    double bd = 0.0;
    int64_t bi = -1;
    for (int64_t r = lane; r < T.n_log; r += 64) {
      const double dx = sf_col(T, SF_EGO_X, r) - x0, dy = sf_col(T, SF_EGO_Y, r) - y0;
      const double d2 = dx * dx + dy * dy;
      if (d2 == d2 && (bi < 0 || d2 < bd)) {
        bd = d2;
        bi = r;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(bd, o, 64);
      const int64_t oi = __shfl_xor(bi, o, 64);
      if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) {
        bd = od;
        bi = oi;
      }
    }
    if (bi < 0) {  // every distance NaN (a non-finite first state): np.nanargmin raises
      sf_write_record(rec, lane, SF_NO_START, -1, 0);
      return;
    }
    T.start = bi;
    T.L = n_track < T.n_log - bi ? n_track : T.n_log - bi;
    T.M = T.start + T.L;
    if (T.L >= 2) {  // np.gradient's uniform-spacing test: (diffx == diffx[0]).all()
      T.dx0 = sf_col(T, SF_FRAME, T.start + 1) - sf_col(T, SF_FRAME, T.start);
      bool differs = false;
      for (int64_t k = lane; k < T.L - 1; k += 64) {
        const double d = sf_col(T, SF_FRAME, T.start + k + 1) - sf_col(T, SF_FRAME, T.start + k);
        differs |= !(d == T.dx0);
      }
      T.uniform = __ballot(differs) == 0ull;
    }
  } else {  // the log as recorded
    T.start = T.n_log;
    T.L = 0;
    T.M = T.n_log;
  }
  const int64_t rep_start = A.merge ? T.start : 0;

  // per-row output: this track's slice, clipped to the buffer
  int64_t ro = 0, cap = 0;
  if (A.rows && A.want_rows) {
    ro = A.row_off[p];
    const int64_t re = A.row_off[p + 1];
    if (ro >= 0 && re <= A.n_out_rows && re > ro) cap = re - ro < T.M ? re - ro : T.M;
  }
  if (cap > 0 && (A.want_rows & SF_ROWS_EGO)) {
    for (int64_t base = 0; base < T.M; base += 64) {
      double ego[7];
      sf_chunk_ego(T, base, lane, lvx, lvy, ego);
      const int64_t r = base + lane;
      if (r < cap)
        for (int k = 0; k < 7; ++k) A.rows[(SF_O_EGO + k) * A.n_out_rows + ro + r] = ego[k];
    }
  }

  // 2. the scenario window [i0, i1] (or to the end)
  const int64_t i0 = sf_first<false>(T, 0, T.M, lane);
  if (i0 < 0) {
    sf_write_record(rec, lane, SF_NO_WINDOW, rep_start, T.L);
    return;
  }
  const int64_t i1 = sf_first<true>(T, i0, T.M, lane);
  const int64_t wend = i1 >= 0 ? i1 + 1 : T.M;

  // 3.-5. one in-order pass over the window, chunks of 64 rows from i0
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = sf_nan();
  const bool dec_is_min = T.scene == SF_STATIC;
  const double dt_def = sf_default_dt(T.scene);
  double n_sub = 0.0, n_ttc = 0.0, n_pet = 0.0, n_jerk = 0.0, n_dec = 0.0, n_yaw = 0.0;
  double s_ttc = 0.0, s_pet = 0.0, s_jerk = 0.0;
  double mn_ttc = inf, mn_pet = inf, mx_jerk = -inf, dec = dec_is_min ? inf : -inf, mx_yaw = -inf;
  bool sub_open = T.scene != SF_UNPREDICTABLE, sub_closed = false;  // wave-uniform
  double a_carry = nan;
  for (int64_t base = i0; base < wend; base += 64) {
    const int64_t r = base + lane;
    const bool active = r < wend;
    double ego[7];
    sf_chunk_ego(T, base, lane, lvx, lvy, ego);
    const double a = T.scene == SF_DYNAMIC ? ego[SF_E_AX] : ego[SF_E_AY];
    double a_prev = __shfl_up(a, 1, 64);
    if (lane == 0) a_prev = a_carry;
    a_carry = __shfl(a, 63, 64);
    double ttc = nan, pet = nan, jerk = nan;
    bool in_sub = active;
    bool hit = false;
    if (active) {
      ttc = sf_ttc(T, r, ego);
      pet = sf_pet(T, r, ego);
      if (r > i0) {  // JERK = diff(a) / dt inside the window (:300-328)
        const double da = a - a_prev;
        if (T.has_time) {
          const double dt = sf_col(T, SF_TIME, r) - sf_col(T, SF_TIME, r - 1);
          jerk = fabs(dt) > SF_EPS_V ? da / dt : nan;
        } else {
          jerk = da / dt_def;
        }
      }
      // 4. the scenario sub-window of main() (:412-456)
      switch (T.scene) {
        case SF_STATIC: {
          const double sx = sf_col(T, SF_SV2_X, r);
          in_sub = sx >= SF_SUB_STATIC_LO && sx <= SF_SUB_STATIC_HI;
          break;
        }
        case SF_DYNAMIC: hit = ego[SF_E_AX] >= SF_SUB_DYNAMIC_AX; break;
        case SF_PREDICTABLE: in_sub = sf_col(T, SF_SV1_X, r) <= SF_SUB_PREDICTABLE_X; break;
        default:
          hit = (sf_col(T, SF_SV1_X, r) - SF_SUB_LANE_X1) * (SF_SUB_LANE_Y2 - SF_SUB_LANE_Y1) -
                (sf_col(T, SF_SV1_Y, r) - SF_SUB_LANE_Y1) * (SF_SUB_LANE_X2 - SF_SUB_LANE_X1) > 0.0;
      }
    }
    if (T.scene == SF_DYNAMIC) {  // rows before the first ego_ax >= 100 (.loc[:first - 1])
      const unsigned long long m = __ballot(hit);
      if (sub_closed) in_sub = false;
      else if (m) {
        in_sub = in_sub && lane < __ffsll((long long)m) - 1;
        sub_closed = true;
      }
    } else if (T.scene == SF_UNPREDICTABLE) {  // from the first row right of the lane line
      const unsigned long long m = __ballot(hit);
      if (!sub_open) {
        if (m) {
          in_sub = in_sub && lane >= __ffsll((long long)m) - 1;
          sub_open = true;
        } else in_sub = false;
      }
    }
    // 5. the statistics over the sub-window (_sub_valid_for_metric :369-380)
    if (in_sub) {
      n_sub += 1.0;
      if (ttc > 0.0) {
        n_ttc += 1.0;
        s_ttc = s_ttc + ttc;
        mn_ttc = ttc < mn_ttc ? ttc : mn_ttc;
        const double d = T.scene == SF_DYNAMIC ? ego[SF_E_AX] : ego[SF_E_AY];
        if (d == d) {
          n_dec += 1.0;
          dec = dec_is_min ? (d < dec ? d : dec) : (d > dec ? d : dec);
        }
        const double yw = ego[SF_E_YAW];
        if (yw == yw) {
          n_yaw += 1.0;
          mx_yaw = yw > mx_yaw ? yw : mx_yaw;
        }
      }
      if (isfinite(pet) && pet >= 0.0) {
        n_pet += 1.0;
        s_pet = s_pet + pet;
        mn_pet = pet < mn_pet ? pet : mn_pet;
      }
      if (isfinite(jerk)) {
        const double j = fabs(jerk);
        n_jerk += 1.0;
        s_jerk = s_jerk + j;
        mx_jerk = j > mx_jerk ? j : mx_jerk;
      }
    }
    if (active && r < cap && (A.want_rows & SF_ROWS_WINDOW)) {
      A.rows[SF_O_TTC * A.n_out_rows + ro + r] = ttc;
      A.rows[SF_O_PET * A.n_out_rows + ro + r] = pet;
      A.rows[SF_O_JERK * A.n_out_rows + ro + r] = jerk;
    }
  }
  n_sub = sf_wave_sum(n_sub);   // counts: exact in float64
  n_ttc = sf_wave_sum(n_ttc);
  n_pet = sf_wave_sum(n_pet);
  n_jerk = sf_wave_sum(n_jerk);
  n_dec = sf_wave_sum(n_dec);
  n_yaw = sf_wave_sum(n_yaw);
  s_ttc = sf_wave_sum(s_ttc);
  s_pet = sf_wave_sum(s_pet);
  s_jerk = sf_wave_sum(s_jerk);
  mn_ttc = sf_wave_min(mn_ttc);
  mn_pet = sf_wave_min(mn_pet);
  mx_jerk = sf_wave_max(mx_jerk);
  dec = dec_is_min ? sf_wave_min(dec) : sf_wave_max(dec);
  mx_yaw = sf_wave_max(mx_yaw);
  if (lane == 0) {
    rec[SF_R_STATUS] = (double)SF_OK;
    rec[SF_R_START] = (double)rep_start;
    rec[SF_R_L] = (double)T.L;
    rec[SF_R_I0] = (double)i0;
    rec[SF_R_I1] = (double)i1;
    rec[SF_R_NWIN] = (double)(wend - i0);
    rec[SF_R_NSUB] = n_sub;
    rec[SF_R_TTC_N] = n_ttc;
    rec[SF_R_TTC_MEAN] = n_ttc > 0.0 ? s_ttc / n_ttc : nan;
    rec[SF_R_TTC_MIN] = n_ttc > 0.0 ? mn_ttc : nan;
    rec[SF_R_PET_N] = n_pet;
    rec[SF_R_PET_MEAN] = n_pet > 0.0 ? s_pet / n_pet : nan;
    rec[SF_R_PET_MIN] = n_pet > 0.0 ? mn_pet : nan;
    rec[SF_R_JERK_N] = n_jerk;
    rec[SF_R_JERK_MEAN] = n_jerk > 0.0 ? s_jerk / n_jerk : nan;
    rec[SF_R_JERK_MAX] = n_jerk > 0.0 ? mx_jerk : nan;
    rec[SF_R_DECEL] = n_dec > 0.0 ? dec : nan;
    rec[SF_R_YAW_MAX] = n_yaw > 0.0 ? mx_yaw : nan;
  }
}

__global__ __launch_bounds__(64 * SF_MAX_WAVES) void safety_kernel(SfArgs A) {
  __shared__ double sf_lds[SF_MAX_WAVES][2][SF_LDS_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  for (int64_t p = (int64_t)blockIdx.x * waves + wave; p < A.P; p += (int64_t)gridDim.x * waves)
    sf_track(A, p, lane, sf_lds[wave][0], sf_lds[wave][1]);
}

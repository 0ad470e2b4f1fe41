// mm_supervisor_dmc.hip -- the "dmc" safety supervisor of merge-multi-agent-v0 (include/mm_supervisor.h).
//
// decentralised_dmc.py:70-193 safety_layer_dmc: priority keys, every controlled vehicle propagated n_points sub-steps with
// its ORIGINAL action (step 1), every HDV propagated behind them (step 1a, a Gauss-Seidel chain), then per controlled vehicle
// in key order a collision scan of its stored points against those of its four lane neighbours and the obstacle and, on the
// first crash, the replacement search of _evaluate_vehicle_action: every available action scored by the sum of
// n_points check_safety_room calls on ONE continuing copy of the original vehicle (step 2).
//
// Two forms behind mm_supervise_dmc, built from the same device functions (stage_*), so that they agree bit for bit:
//   literal (MM_DMC_LITERAL): one lane per env runs the stages in the Python's order.
//   default: four launches that are lane-parallel where the algorithm is --
//     dmc_propagate  one lane per (env, slot): the key and the n_points-step trajectory of a controlled vehicle
//     dmc_scan       one lane per env: key order, the HDV chain, neighbours + collision scan in key order; every
//                    (crashing vehicle, available action) pair is appended to one work list for the whole batch
//     dmc_score      one lane per listed pair: the n_points (n_points + 1) / 2 dependent controller steps of a candidate
//     dmc_finish     one lane per (env, slot): first maximum, new_actions, n_draws, trace
// Everything between the launches lives in the caller's scratch buffer as planes [plane][E * N], so consecutive lanes of
// dmc_propagate / dmc_finish touch consecutive doubles.  Every loop runs to a bound fixed by n_points and N.
#include "mm_supervisor_dev.h"
#include "../../include/mm_supervisor.h"

#include "mm_handle.h"

namespace mm {
namespace dmc {
using namespace mm::sup;

// trace fields per slot (include/mm_supervisor.h); inside the scratch buffer they are planes
enum { T_POS = 0, T_KEY, T_CRASH, T_FL, T_RR, T_FR, T_RL, T_MASK, T_ROOM, T_EX = T_ROOM + 5, T_EY, T_EH, T_EV, T_HS, T_HA, T_STAND };
static_assert(T_STAND + 1 == MM_DMC_TRACE_DOUBLES, "trace layout");
constexpr int kTraj = 4;       // per trajectory point: x, y, heading, speed
constexpr int kMaxPoints = 128;  // the candidate's first n_points x live in LDS: 64 lanes x n_points doubles <= 64 KiB

struct Args {
  const double *f64;  // [MM_F_COUNT][E*N]
  const uint8_t *u8;  // [MM_B_COUNT][E*N]
  const int32_t *ep;  // [MM_E_COUNT][E]
  const uint64_t *seed;
  const int32_t *actions;
  const double *uniforms;
  int stride;
  double *scr;
  int32_t *new_actions, *n_draws;
  double *trace;
  int E, N, n_points;
  double dt, headway_time;
};

// the scratch buffer: trajectory planes [t][4], the trace planes, the key order [E][N], then the work list (int32) and its count
struct Scr {
  double *p;
  long long EN;
  int np;
  MM_DEV double &traj(int t, int f, long long a) const { return p[((long long)t * kTraj + f) * EN + a]; }
  MM_DEV double &tr(int k, long long a) const { return p[((long long)np * kTraj + k) * EN + a]; }
  MM_DEV double &ord(long long a) const { return p[((long long)np * kTraj + MM_DMC_TRACE_DOUBLES) * EN + a]; }
  MM_DEV int32_t *items() const { return (int32_t *)(p + ((long long)np * kTraj + MM_DMC_TRACE_DOUBLES + 1) * EN); }
  MM_DEV int32_t *count() const { return items() + 5 * EN; }
};
MM_DEV Scr scr_of(const Args &a) { return Scr{a.scr, (long long)a.E * a.N, a.n_points}; }

struct Env {  // what every stage needs of one env
  long long b0, EN;
  int e, ncav, nv;
};
MM_DEV Env env_of(const Args &a, int e) {
  Env v;
  v.e = e;
  v.EN = (long long)a.E * a.N;
  v.b0 = (long long)e * a.N;
  int ncav = 0, nhdv = 0;
  for (int s = 0; s < a.N; s++) {
    const int k = a.u8[MM_B_KIND * v.EN + v.b0 + s];
    ncav += k == 1;
    nhdv += k == 2;
  }
  // vehicles of an env are a prefix, CAVs first (mm_abi.h): slots 0..ncav-1 are controlled_vehicles, 0..nv-1 road.vehicles
  v.ncav = ncav;
  v.nv = ncav + nhdv;
  return v;
}
MM_DEV double F(const Args &a, const Env &v, int plane, int s) { return a.f64[plane * v.EN + v.b0 + s]; }
MM_DEV int B(const Args &a, const Env &v, int plane, int s) { return (int)a.u8[plane * v.EN + v.b0 + s]; }

// np.random.rand() number d of the env: CAV i draws d = i, the j-th HDV d = ncav + 2 j and ncav + 2 j + 1
template <bool PHILOX>
MM_DEV double draw(const Args &a, int e, int d) {
  if constexpr (!PHILOX) {
    return d < a.stride ? a.uniforms[(long long)e * a.stride + d] : 0.5;
  } else {
    return philox_draw(d, (uint32_t)a.ep[MM_E_EPISODE * a.E + e], (uint32_t)a.ep[MM_E_STEPS * a.E + e], a.seed[e]);
  }
}

// every trace field of slot s at its "nothing happened" value; an absent slot keeps these
MM_DEV void stage_init(const Args &a, const Env &v, int s) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  const double nan = __builtin_nan("");
  S.tr(T_POS, i) = -1; S.tr(T_KEY, i) = nan; S.tr(T_CRASH, i) = -1;
  S.tr(T_FL, i) = -1; S.tr(T_RR, i) = -1; S.tr(T_FR, i) = -1; S.tr(T_RL, i) = -1;
  S.tr(T_MASK, i) = 0;
  for (int c = 0; c < 5; c++) S.tr(T_ROOM + c, i) = nan;
  const bool present = s < v.nv;  // the copy's vehicle before anything moves (an HDV later than the one being generated)
  S.tr(T_EX, i) = present ? F(a, v, MM_F_X, s) : nan; S.tr(T_EY, i) = present ? F(a, v, MM_F_Y, s) : nan;
  S.tr(T_EH, i) = present ? F(a, v, MM_F_HEADING, s) : nan; S.tr(T_EV, i) = present ? F(a, v, MM_F_SPEED, s) : nan;
  S.tr(T_HS, i) = nan; S.tr(T_HA, i) = nan;
  S.tr(T_STAND, i) = S.tr(T_EX, i);
  S.ord(i) = s;  // (a valid slot whatever stage_order makes of NaN keys)
}

// the priority key of controlled vehicle s (decentralised_dmc.py:89-116)
template <bool PHILOX>
MM_DEV void stage_key(const Args &a, const Env &v, int s) {
  const double p = priority_number(B(a, v, MM_B_LANE, s), F(a, v, MM_F_X, s), F(a, v, MM_F_Y, s), F(a, v, MM_F_SPEED, s), v.nv,
                                   a.headway_time, [&](int u) { return B(a, v, MM_B_LANE, u); },
                                   [&](int u) { return F(a, v, MM_F_X, u); });
  scr_of(a).tr(T_KEY, v.b0 + s) = p + draw<PHILOX>(a, v.e, s) * 0.001;
}

// step 1 for controlled vehicle s: n_points x mdp_controller with its original action, re-applied at every sub-step
MM_DEV void stage_propagate(const Args &a, const Env &v, int s) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  double x = F(a, v, MM_F_X, s), y = F(a, v, MM_F_Y, s), h = F(a, v, MM_F_HEADING, s), sp = F(a, v, MM_F_SPEED, s);
  double ts = F(a, v, MM_F_TARGET_SPEED, s);
  int tl = B(a, v, MM_B_TARGET_LANE, s);
  const bool cr = B(a, v, MM_B_CRASHED, s) != 0;
  const int act = a.actions[i];
  for (int t = 0; t < a.n_points; t++) {
    mdp_step(x, y, h, sp, ts, tl, cr, act, a.dt);
    S.traj(t, 0, i) = x; S.traj(t, 1, i) = y; S.traj(t, 2, i) = h; S.traj(t, 3, i) = sp;
  }
  S.tr(T_EX, i) = x; S.tr(T_EY, i) = y; S.tr(T_EH, i) = h; S.tr(T_EV, i) = sp;
  S.tr(T_STAND, i) = x;
}

// key order: position = the number of keys before it (stable, as the priority kernel's insertion sort)
MM_DEV void stage_order(const Args &a, const Env &v) {
  const Scr S = scr_of(a);
  for (int i = 0; i < v.ncav; i++) {
    const double k = S.tr(T_KEY, v.b0 + i);
    int pos = 0;
    for (int j = 0; j < v.ncav; j++) {
      const double kj = S.tr(T_KEY, v.b0 + j);
      pos += (kj < k) || (j < i && !(kj > k));
    }
    S.tr(T_POS, v.b0 + i) = pos;
    S.ord(v.b0 + pos) = i;
  }
}

// step 1a for HDV s (decentralised_dmc.py:130-137): generate_actions once on the copy as it is now -- every CAV and every
// earlier HDV at the END of its horizon, later HDVs at their start (the T_E* planes hold exactly that) -- then n_points x
// idm_controller.  A crashed HDV still draws; its points alias its live position, which never moves.
template <bool PHILOX>
MM_DEV void stage_hdv(const Args &a, const Env &v, int s) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  const int d = v.ncav + 2 * (s - v.ncav);
  const double u1 = draw<PHILOX>(a, v.e, d), u2 = draw<PHILOX>(a, v.e, d + 1);
  double x = F(a, v, MM_F_X, s), y = F(a, v, MM_F_Y, s), h = F(a, v, MM_F_HEADING, s), sp = F(a, v, MM_F_SPEED, s);
  double steer, acc;
  int front;
  hdv_generate(s, B(a, v, MM_B_LANE, s), v.nv, x, y, h, sp, F(a, v, MM_F_TARGET_SPEED, s), u1, u2,
               [&](int u, double &ux, double &uy, double &uh, double &uv) {
                 ux = S.tr(T_EX, v.b0 + u); uy = S.tr(T_EY, v.b0 + u); uh = S.tr(T_EH, v.b0 + u); uv = S.tr(T_EV, v.b0 + u);
               },
               steer, acc, front);
  S.tr(T_HS, i) = steer; S.tr(T_HA, i) = acc;
  const bool cr = B(a, v, MM_B_CRASHED, s) != 0;
  for (int t = 0; t < a.n_points; t++) {
    if (!cr) idm_move(x, y, h, sp, steer, acc, a.dt);
    S.traj(t, 0, i) = x; S.traj(t, 1, i) = y; S.traj(t, 2, i) = h; S.traj(t, 3, i) = sp;
  }
  S.tr(T_EX, i) = x; S.tr(T_EY, i) = y; S.tr(T_EH, i) = h; S.tr(T_EV, i) = sp;
  S.tr(T_STAND, i) = x;
}

// surrounding_vehicles(vehicle, q) (road.py:294-346) with the copy's CURRENT x (T_STAND) and ORIGINAL lanes
MM_DEV void query(const Args &a, const Env &v, const Scr &S, int ego, int q, int &front, int &rear) {
  const double s = S.tr(T_STAND, v.b0 + ego);
  bool hf = false, hr = false;
  double sf = 0, sr = 0;
  front = rear = -1;
  for (int u = 0; u < v.nv; u++) {
    if (u == ego || !accepts(q, B(a, v, MM_B_LANE, u))) continue;
    const double su = S.tr(T_STAND, v.b0 + u);
    if (s <= su && (!hf || su <= sf)) { sf = su; front = u; hf = true; }
    if (su < s && (!hr || su > sr)) { sr = su; rear = u; hr = true; }
  }
}

// step 2 up to the crash for controlled vehicle s (decentralised_dmc.py:141-179, :32-47): neighbours, available actions,
// the first point that collides.  Leaves the vehicle standing at that point for later queries.  Returns crash_t (-1: none).
MM_DEV int stage_scan(const Args &a, const Env &v, int s) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  const int lane = B(a, v, MM_B_LANE, s);
  int fl = -1, rl = -1, fr = -1, rr = -1;  // lane cases of central_layer.py:85-110
  if (is_main(lane)) {
    query(a, v, S, s, lane, fl, rl);
    if (lane == MM_LANE_BC0) query(a, v, S, s, MM_LANE_BC1, fr, rr);
    else if (lane == MM_LANE_AB0 && S.tr(T_STAND, i) > 220.0) query(a, v, S, s, MM_LANE_KB0, fr, rr);
  } else {
    query(a, v, S, s, lane, fr, rr);
    if (lane == MM_LANE_BC1) query(a, v, S, s, MM_LANE_BC0, fl, rl);
    else if (lane == MM_LANE_KB0) query(a, v, S, s, MM_LANE_AB0, fl, rl);
  }
  S.tr(T_FL, i) = fl; S.tr(T_RR, i) = rr; S.tr(T_FR, i) = fr; S.tr(T_RL, i) = rl;
  int avail[5];
  const int na = available_actions(lane, F(a, v, MM_F_X, s), F(a, v, MM_F_Y, s), B(a, v, MM_B_SPEED_INDEX, s), avail);
  int mask = 0;
#pragma unroll
  for (int c = 0; c < 5; c++)
    if (c < na) mask |= 1 << avail[c];
  S.tr(T_MASK, i) = mask;
  int crash_t = -1;
  for (int t = 0; t < a.n_points; t++) {
    const double ex = S.traj(t, 0, i), ey = S.traj(t, 1, i), eh = S.traj(t, 2, i);
    bool hit = false;
    const int nb[4] = {fl, rr, fr, rl};  // neighbours = [v_fl, v_rr, v_fr, v_rl]
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int o = nb[k];
      if (o >= 0 && colliding(ex, ey, eh, S.traj(t, 0, v.b0 + o), S.traj(t, 1, v.b0 + o), S.traj(t, 2, v.b0 + o), kVehLength, kVehWidth))
        hit = true;
    }
    if (colliding(ex, ey, eh, kObstX, kObstY, 0.0, 2.0, 2.0)) hit = true;
    if (hit && crash_t < 0) crash_t = t;
  }
  S.tr(T_CRASH, i) = crash_t;
  if (crash_t >= 0) S.tr(T_STAND, i) = S.traj(crash_t, 0, i);
  return crash_t;
}

// the score of candidate `action` for crashing vehicle s (decentralised_dmc.py:52-61): ONE copy of the original vehicle
// runs call k = 0..n_points-1 of check_safety_room (abstract.py:242-280) without a reset, so call k takes k + 1 FURTHER
// controller steps and distance_to_merging_end from that continuing state, while the x it compares are the copy's FIRST
// points 0..k (px, this lane's column of LDS, stride 64) and the neighbours' points 0..k.
MM_DEV void stage_score(const Args &a, const Env &v, int s, int action, double *px) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  const int np = a.n_points;
  const int lane = B(a, v, MM_B_LANE, s);
  const int fl = (int)S.tr(T_FL, i), rr = (int)S.tr(T_RR, i), fr = (int)S.tr(T_FR, i), rl = (int)S.tr(T_RL, i);
  double x = F(a, v, MM_F_X, s), y = F(a, v, MM_F_Y, s), h = F(a, v, MM_F_HEADING, s), sp = F(a, v, MM_F_SPEED, s);
  double ts = F(a, v, MM_F_TARGET_SPEED, s);
  int tl = B(a, v, MM_B_TARGET_LANE, s);
  const bool cr = B(a, v, MM_B_CRASHED, s) != 0;
  const bool lane_change = action == 0 || action == 2;
  const int lead = is_main(lane) ? fl : fr;
  double sum = 0;
  int g = 0;  // controller steps taken so far
  for (int k = 0; k < np; k++) {
    double rmin = 0;
    for (int t = 0; t <= k; t++) {
      mdp_step(x, y, h, sp, ts, tl, cr, action, a.dt);
      if (g < np) px[g * 64] = x;
      g++;
      double room = lane == MM_LANE_BC1 ? 420.0 - x : 100.0;  // distance_to_merging_end of the continuing copy
      const double own = px[t * 64];
      if (lane_change) {
        const int nb[4] = {fl, rr, fr, rl};
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (nb[q] >= 0) {
            const double d = fabs(S.traj(t, 0, v.b0 + nb[q]) - own);
            if (d <= room) room = d;
          }
      } else if (lead >= 0) {
        const double d = S.traj(t, 0, v.b0 + lead) - own;
        if (d <= room) room = d;
      }
      if (t == 0 || room < rmin) rmin = room;
    }
    sum += rmin;
  }
  S.tr(T_ROOM + action, i) = sum;
}

// the first maximum over the available actions in the reference's list order (IDLE, LEFT, RIGHT, FASTER, SLOWER)
MM_DEV int stage_pick(const Args &a, const Env &v, int s) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  const int mask = (int)S.tr(T_MASK, i);
  int best = -1;
  double best_room = 0;
  const int order[5] = {1, 0, 2, 3, 4};
#pragma unroll
  for (int c = 0; c < 5; c++) {
    const int ac = order[c];
    if (!((mask >> ac) & 1)) continue;
    const double r = S.tr(T_ROOM + ac, i);
    if (best < 0 || r > best_room) { best = ac; best_room = r; }
  }
  return best;
}

// new_actions, n_draws and the caller's trace of slot s
MM_DEV void stage_output(const Args &a, const Env &v, int s) {
  const Scr S = scr_of(a);
  const long long i = v.b0 + s;
  int act = a.actions[i];
  if (s < v.ncav && S.tr(T_CRASH, i) >= 0) act = stage_pick(a, v, s);
  a.new_actions[i] = act;
  if (s == 0 && a.n_draws) a.n_draws[v.e] = v.ncav + 2 * (v.nv - v.ncav);
  if (a.trace)
    for (int k = 0; k < MM_DMC_TRACE_DOUBLES; k++) a.trace[i * MM_DMC_TRACE_DOUBLES + k] = S.tr(k, i);
}

// ---- the literal form: one lane per env, the Python's order ----
template <bool PHILOX>
__global__ void __launch_bounds__(64) dmc_literal_kernel(Args a) {
  extern __shared__ double lds[];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.E) return;
  const Env v = env_of(a, e);
  const Scr S = scr_of(a);
  for (int s = 0; s < a.N; s++) stage_init(a, v, s);
  for (int s = 0; s < v.ncav; s++) stage_key<PHILOX>(a, v, s);
  stage_order(a, v);
  for (int p = 0; p < v.ncav; p++) stage_propagate(a, v, (int)S.ord(v.b0 + p));
  for (int s = v.ncav; s < v.nv; s++) stage_hdv<PHILOX>(a, v, s);
  for (int p = 0; p < v.ncav; p++) {
    const int s = (int)S.ord(v.b0 + p);
    if (stage_scan(a, v, s) < 0) continue;
    const int mask = (int)S.tr(T_MASK, v.b0 + s);
    for (int ac = 0; ac < 5; ac++)
      if ((mask >> ac) & 1) stage_score(a, v, s, ac, lds + threadIdx.x);
  }
  for (int s = 0; s < a.N; s++) stage_output(a, v, s);
}

// ---- the default form ----
template <bool PHILOX>
__global__ void __launch_bounds__(256) dmc_propagate_kernel(Args a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *scr_of(a).count() = 0;
  if (i >= (long long)a.E * a.N) return;
  const Env v = env_of(a, (int)(i / a.N));
  const int s = (int)(i % a.N);
  stage_init(a, v, s);
  if (s >= v.ncav) return;
  stage_key<PHILOX>(a, v, s);
  stage_propagate(a, v, s);
}

template <bool PHILOX>
__global__ void __launch_bounds__(64) dmc_scan_kernel(Args a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.E) return;
  const Env v = env_of(a, e);
  const Scr S = scr_of(a);
  stage_order(a, v);
  for (int s = v.ncav; s < v.nv; s++) stage_hdv<PHILOX>(a, v, s);
  for (int p = 0; p < v.ncav; p++) {
    const int s = (int)S.ord(v.b0 + p);
    if (stage_scan(a, v, s) < 0) continue;
    // every (crashing vehicle, candidate) pair joins the batch's work list, so that dmc_score's waves are full
    const int mask = (int)S.tr(T_MASK, v.b0 + s);
    const int at = atomicAdd(S.count(), __popc(mask));
    int n = 0;
    for (int ac = 0; ac < 5; ac++)
      if ((mask >> ac) & 1) S.items()[at + n++] = (int)(v.b0 + s) * 8 + ac;  // (E * N * 8 < 2^31: checked by the entry)
  }
}

__global__ void __launch_bounds__(64) dmc_score_kernel(Args a) {
  extern __shared__ double lds[];
  const Scr S = scr_of(a);
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= *S.count()) return;
  const int item = S.items()[j];
  const long long i = item >> 3;
  const Env v = env_of(a, (int)(i / a.N));
  stage_score(a, v, (int)(i % a.N), item & 7, lds + threadIdx.x);
}

__global__ void __launch_bounds__(256) dmc_finish_kernel(Args a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.E * a.N) return;
  const Env v = env_of(a, (int)(i / a.N));
  stage_output(a, v, (int)(i % a.N));
}

}  // namespace dmc
}  // namespace mm

static int32_t dmc_points(int32_t n_step, int32_t sub_steps) {
  const int64_t np = (int64_t)n_step * sub_steps;
  return n_step < 1 || sub_steps < 1 || np > mm::dmc::kMaxPoints ? 0 : (int32_t)np;
}
static uint64_t dmc_scratch_need(int32_t E, int32_t N, int32_t np) {
  const uint64_t EN = (uint64_t)E * (uint64_t)N;
  // trajectory + trace + order planes, then 5 E N work items and their count as int32, rounded up to doubles
  return 8ull * (EN * (uint64_t)(mm::dmc::kTraj * np + MM_DMC_TRACE_DOUBLES + 1) + (5 * EN + 1 + 1) / 2);
}

extern "C" int32_t mm_supervise_dmc_scratch_bytes(int32_t E, int32_t N, int32_t n_step, int32_t sub_steps, uint64_t *bytes) {
  if (!bytes || E <= 0 || N <= 0 || N > MM_MAX_AGENTS || (int64_t)E * N * 8 > INT32_MAX || !dmc_points(n_step, sub_steps))
    return MM_ERR_INVALID_ARG;
  *bytes = dmc_scratch_need(E, N, dmc_points(n_step, sub_steps));
  return MM_OK;
}

extern "C" int32_t mm_supervise_dmc(MMHandle hd, int32_t n_step, uint32_t flags, const int32_t *actions, const double *uniforms,
                                    int32_t uniform_stride, void *scratch, uint64_t scratch_bytes, int32_t *new_actions,
                                    int32_t *n_draws, double *trace, MMStream stream) {
  if (!hd) return MM_ERR_INVALID_ARG;
  const MMHandleHead *h = mm_handle_head(hd);
  const MMConfig &c = h->cfg;
  const int32_t np = dmc_points(n_step, c.policy_frequency > 0 ? c.simulation_frequency / c.policy_frequency : 0);
  if (c.env_kind != MM_ENV_V0 || n_step < 1 || np < 1 || (flags & ~MM_DMC_LITERAL) || !actions || !new_actions || !scratch ||
      ((uintptr_t)scratch & 7u) || (uniforms && uniform_stride < 2 * h->N) || (int64_t)h->E * h->N * 8 > INT32_MAX ||
      scratch_bytes < dmc_scratch_need(h->E, h->N, np))
    return MM_ERR_INVALID_ARG;
  mm::dmc::Args a;
  a.f64 = (const double *)(h->state + h->lay.f64_offset);
  a.u8 = h->state + h->lay.u8_offset;
  a.ep = (const int32_t *)(h->state + h->lay.env_offset);
  a.seed = (const uint64_t *)(h->state + h->lay.seed_offset);
  a.actions = actions;
  a.uniforms = uniforms;
  a.stride = uniform_stride;
  a.scr = (double *)scratch;
  a.new_actions = new_actions;
  a.n_draws = n_draws;
  a.trace = trace;
  a.E = h->E; a.N = h->N; a.n_points = np;
  a.dt = 1.0 / c.simulation_frequency;
  a.headway_time = c.headway_time;
  const hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)np * 64 * sizeof(double);  // stage_score's px column per lane
  const long long EN = (long long)h->E * h->N;
  const dim3 per_env((unsigned)((h->E + 63) / 64)), per_slot((unsigned)((EN + 255) / 256)), per_pair((unsigned)((5 * EN + 63) / 64));
  if (flags & MM_DMC_LITERAL) {
    if (uniforms) hipLaunchKernelGGL(mm::dmc::dmc_literal_kernel<false>, per_env, dim3(64), lds, st, a);
    else hipLaunchKernelGGL(mm::dmc::dmc_literal_kernel<true>, per_env, dim3(64), lds, st, a);
  } else {
    if (uniforms) {
      hipLaunchKernelGGL(mm::dmc::dmc_propagate_kernel<false>, per_slot, dim3(256), 0, st, a);
      hipLaunchKernelGGL(mm::dmc::dmc_scan_kernel<false>, per_env, dim3(64), 0, st, a);
    } else {
      hipLaunchKernelGGL(mm::dmc::dmc_propagate_kernel<true>, per_slot, dim3(256), 0, st, a);
      hipLaunchKernelGGL(mm::dmc::dmc_scan_kernel<true>, per_env, dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(mm::dmc::dmc_score_kernel, per_pair, dim3(64), lds, st, a);
    hipLaunchKernelGGL(mm::dmc::dmc_finish_kernel, per_slot, dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

// mm_supervisor.hip -- the "priority" safety supervisor of merge-multi-agent-v0 (include/mm_supervisor.h).
//
// central_layer.py:16-178 safety_supervisor, literally, one lane per env: priority keys, then for each controlled vehicle
// in priority order an n_points-sub-step lookahead of it and its four lane neighbours on a copy of the env whose vehicles
// move in place, with the crash -> best-safety-room replacement of abstract.py:242-280.  The lookahead copy (live state
// and every stored trajectory point) lives in the caller's scratch buffer, laid out [field][slot][env] so that the lanes
// of a wave touch consecutive doubles.  The arithmetic is the step kernel's (mm_device.h, include/mm_math.h); only the
// integrator of mdp_controller.py:19-64 differs from Vehicle.step (no speed floor, no lane update).  The helpers it shares
// with the "dmc" supervisor (mm_supervisor_dmc.hip) are in mm_supervisor_dev.h.
#include "mm_supervisor_dev.h"
#include "../../include/mm_supervisor.h"

#include "mm_handle.h"

#include <string.h>

namespace mm {
namespace sup {

// live fields of the copy: x, y, heading, speed, target speed, target lane, crashed, len(trajectories), and an HDV's
// vehicle.action of its generate_actions call (steering, acceleration)
constexpr int kLive = 10;
enum { LX = 0, LY, LH, LV, LTS, LTL, LCR, LLEN, LHS, LHA };
// per trajectory point: x, y, heading, speed.  x = NaN: the point of a crashed HDV, whose position idm_controller
// appends WITHOUT a copy (idm_controller.py:42-44): it reads as the vehicle's live position
constexpr int kTraj = 4;

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
  int E, N, n_points;
  double dt, headway_time;
};

struct View {  // one env's slice of the scratch buffer
  double *p;
  long long E;
  int N;
  MM_DEV double &live(int f, int v) const { return p[((long long)f * N + v) * E]; }
  MM_DEV double &traj(int t, int f, int v) const { return p[((long long)kLive * N + ((long long)t * kTraj + f) * N + v) * E]; }
};

// PHILOX: the device draws (uniforms == NULL) -- a compile-time choice, not a branch inside draw().  As a run-time test of the
// (wave-uniform) pointer the compiler kept the answer as a lane mask formed inside the priority-key loop, i.e. under the exec
// mask of that loop's LAST trip: only the lanes whose env has the most controlled vehicles of the wave.  A later draw by lanes
// outside that mask (an HDV's generate_actions in a ragged wave) then took the recorded-uniforms path and got its 0.5 filler
// instead of the Philox value (found by tests/test_supervisor_twin_gpu.py; DESIGN.md "Supervisor parity").
template <bool PHILOX>
__global__ void __launch_bounds__(64) supervise_kernel(Args a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.E) return;
  const int N = a.N;
  const long long EN = (long long)a.E * N, b0 = (long long)e * N;
  auto F = [&](int plane, int v) { return a.f64[plane * EN + b0 + v]; };
  auto B = [&](int plane, int v) { return (int)a.u8[plane * EN + b0 + v]; };
  int act[MM_MAX_AGENTS];
  int ncav = 0, nhdv = 0;
  for (int v = 0; v < N; v++) {
    act[v] = a.actions[b0 + v];
    const int k = B(MM_B_KIND, v);
    ncav += k == 1;
    nhdv += k == 2;
  }
  if (ncav == 0) {  // no controlled vehicle: nothing to supervise
    for (int v = 0; v < N; v++) a.new_actions[b0 + v] = act[v];
    if (a.n_draws) a.n_draws[e] = 0;
    return;
  }
  // vehicles of an env are a prefix, CAVs first (mm_abi.h): slots 0..ncav-1 are controlled_vehicles, 0..nv-1 road.vehicles
  const int n = ncav, nv = ncav + nhdv;
  const View S{a.scr + e, a.E, N};
  int nd = 0;  // np.random.rand() values drawn so far

  // ---- priority keys (central_layer.py:32-65): the smallest key is taken first ----
  int order[MM_MAX_AGENTS];
  double key[MM_MAX_AGENTS];
  const uint64_t seed = a.seed[e];
  const uint32_t episode = (uint32_t)a.ep[MM_E_EPISODE * a.E + e], steps = (uint32_t)a.ep[MM_E_STEPS * a.E + e];
  auto draw = [&]() {
    const int d = nd++;
    if constexpr (!PHILOX) {
      return d < a.stride ? a.uniforms[(long long)e * a.stride + d] : 0.5;  // (at most 9 N draws: see header)
    } else {
      return philox_draw(d, episode, steps, seed);
    }
  };
  for (int i = 0; i < n; i++) {
    const double p = priority_number(B(MM_B_LANE, i), F(MM_F_X, i), F(MM_F_Y, i), F(MM_F_SPEED, i), nv, a.headway_time,
                                     [&](int v) { return B(MM_B_LANE, v); }, [&](int v) { return F(MM_F_X, v); });
    key[i] = p + draw() * 0.001;
    order[i] = i;
  }
  for (int i = 1; i < n; i++) {  // insertion sort, stable: PriorityQueue order for distinct keys
    const int o = order[i];
    const double k = key[o];
    int j = i - 1;
    while (j >= 0 && key[order[j]] > k) { order[j + 1] = order[j]; j--; }
    order[j + 1] = o;
  }

  // ---- the lookahead copy (central_layer.py:22-29) ----
  for (int v = 0; v < nv; v++) {
    S.live(LX, v) = F(MM_F_X, v); S.live(LY, v) = F(MM_F_Y, v); S.live(LH, v) = F(MM_F_HEADING, v);
    S.live(LV, v) = F(MM_F_SPEED, v); S.live(LTS, v) = F(MM_F_TARGET_SPEED, v);
    S.live(LTL, v) = B(MM_B_TARGET_LANE, v); S.live(LCR, v) = B(MM_B_CRASHED, v); S.live(LLEN, v) = 0;
    S.live(LHS, v) = 0; S.live(LHA, v) = 0;
  }
  const int np = a.n_points;
  const double dt = a.dt;
  // one sub-step of vehicle v in the copy with `action`, appending its trajectory point
  auto step_live = [&](int v, int action) {
    double x = S.live(LX, v), y = S.live(LY, v), h = S.live(LH, v), sp = S.live(LV, v), ts = S.live(LTS, v);
    const int t = (int)S.live(LLEN, v);
    if (t >= np) return;  // (cannot happen: every vehicle holds 0 or n_points points when an ego starts)
    int tl = (int)S.live(LTL, v);
    mdp_step(x, y, h, sp, ts, tl, S.live(LCR, v) != 0, action, dt);
    S.live(LX, v) = x; S.live(LY, v) = y; S.live(LH, v) = h; S.live(LV, v) = sp; S.live(LTS, v) = ts; S.live(LTL, v) = tl;
    S.traj(t, 0, v) = x; S.traj(t, 1, v) = y; S.traj(t, 2, v) = h; S.traj(t, 3, v) = sp;
    S.live(LLEN, v) = t + 1;
  };
  // a stored trajectory point's position (the live one for an aliased point of a crashed HDV)
  auto tx = [&](int t, int v) { const double x = S.traj(t, 0, v); return x != x ? S.live(LX, v) : x; };
  auto ty = [&](int t, int v) { return S.traj(t, 0, v) != S.traj(t, 0, v) ? S.live(LY, v) : S.traj(t, 1, v); };
  // idm_controller(v, env_copy, v.action) (idm_controller.py:41-56)
  auto idm_step = [&](int v) {
    const int t = (int)S.live(LLEN, v);
    if (t >= np) return;
    const double h = S.live(LH, v), sp = S.live(LV, v);
    if (S.live(LCR, v) != 0) {  // appended without moving, position not copied
      S.traj(t, 0, v) = __builtin_nan(""); S.traj(t, 1, v) = __builtin_nan(""); S.traj(t, 2, v) = h; S.traj(t, 3, v) = sp;
      S.live(LLEN, v) = t + 1;
      return;
    }
    double x = S.live(LX, v), y = S.live(LY, v), hh = h, vv = sp, acc = S.live(LHA, v);
    idm_move(x, y, hh, vv, S.live(LHS, v), acc, dt);  // (the clipped acceleration persists)
    S.live(LHA, v) = acc;
    S.live(LX, v) = x; S.live(LY, v) = y; S.live(LH, v) = hh; S.live(LV, v) = vv;
    S.traj(t, 0, v) = x; S.traj(t, 1, v) = y; S.traj(t, 2, v) = hh; S.traj(t, 3, v) = vv;
    S.live(LLEN, v) = t + 1;
  };
  // generate_actions (idm_controller.py:59-76): IDM behind the front vehicle of its own (original) lane, MOBIL, and two
  // draws scaling steering and acceleration.  change_lane_policy returns the vehicle's lane in both of its branches: when
  // lane != target lane directly (:99-111: the abort test `v is v.lane_index != ...` is always false), otherwise after
  // MOBIL, which never accepts -- its "new" and "old" neighbours come from the same own-lane query (:137,144), so
  // self_pred_a == self_a and the jerk is 0 < LANE_CHANGE_MIN_ACC_GAIN (an HDV has no route, :146)
  auto generate_actions = [&](int v) {
    const int L = B(MM_B_LANE, v);
    const double x = S.live(LX, v), y = S.live(LY, v), h = S.live(LH, v), sp = S.live(LV, v);
    double tl = S.live(LTL, v);
    if (lane_after_end((int)tl, x)) S.live(LTL, v) = next_lane((int)tl, x, y);  // follow_road :78-84
    const double u1 = draw(), u2 = draw();
    double steer, acc;
    int front;
    hdv_generate(v, L, nv, x, y, h, sp, S.live(LTS, v), u1, u2,
                 [&](int u, double &ux, double &uy, double &uh, double &uv) {
                   ux = S.live(LX, u); uy = S.live(LY, u); uh = S.live(LH, u); uv = S.live(LV, u);
                 },
                 steer, acc, front);
    S.live(LHS, v) = steer;
    S.live(LHA, v) = acc;
  };
  auto reset_live = [&](int v) {  // copy.deepcopy(env.controlled_vehicles[index]): the original, no trajectory
    S.live(LX, v) = F(MM_F_X, v); S.live(LY, v) = F(MM_F_Y, v); S.live(LH, v) = F(MM_F_HEADING, v);
    S.live(LV, v) = F(MM_F_SPEED, v); S.live(LTS, v) = F(MM_F_TARGET_SPEED, v);
    S.live(LTL, v) = B(MM_B_TARGET_LANE, v); S.live(LCR, v) = B(MM_B_CRASHED, v); S.live(LLEN, v) = 0;
  };
  // surrounding_vehicles(vehicle, q) (road.py:294-346) with the copy's CURRENT x and ORIGINAL lanes
  auto query = [&](int ego, int q, int &front, int &rear) {
    const double s = S.live(LX, ego);
    bool hf = false, hr = false;
    double sf = 0, sr = 0;
    front = rear = -1;
    for (int v = 0; v < nv; v++) {
      if (v == ego || !accepts(q, B(MM_B_LANE, v))) continue;
      const double sv = S.live(LX, v);
      if (s <= sv && (!hf || sv <= sf)) { sf = sv; front = v; hf = true; }
      if (sv < s && (!hr || sv > sr)) { sr = sv; rear = v; hr = true; }
    }
  };

  for (int i = 0; i < n; i++) {
    const int idx = order[i];
    bool first_change = true;
    if ((int)S.live(LLEN, idx) == np) reset_live(idx);  // stepped before as someone's neighbour (:72-78)
    // _get_available_actions (abstract.py:219-240) of the (unstepped) ego: IDLE, side lanes, FASTER, SLOWER
    const int lane = B(MM_B_LANE, idx);
    int avail[5];
    const int na = available_actions(lane, S.live(LX, idx), S.live(LY, idx), B(MM_B_SPEED_INDEX, idx), avail);
    // neighbours by lane (:85-110): nb = {v_fl, v_rl, v_fr, v_rr}
    int nb[4] = {-1, -1, -1, -1};
    if (is_main(lane)) {
      query(idx, lane, nb[0], nb[1]);
      if (lane == MM_LANE_BC0) query(idx, MM_LANE_BC1, nb[2], nb[3]);
      else if (lane == MM_LANE_AB0 && S.live(LX, idx) > 220.0) query(idx, MM_LANE_KB0, nb[2], nb[3]);
    } else {
      query(idx, lane, nb[2], nb[3]);
      if (lane == MM_LANE_BC1) query(idx, MM_LANE_BC0, nb[0], nb[1]);
      else if (lane == MM_LANE_KB0) query(idx, MM_LANE_AB0, nb[0], nb[1]);
    }
    const int upd[5] = {nb[0], nb[2], idx, nb[1], nb[3]};  // [v_fl, v_fr, vehicle, v_rl, v_rr]
    for (int t = 0; t < np; t++) {
      for (int k = 0; k < 5; k++) {
        const int v = upd[k];
        if (v < 0) continue;
        if (v != idx && (int)S.live(LLEN, v) == np && i != 0) continue;  // stepped before: keeps its trajectory
        if (v >= n) {  // an HDV (type(v) is IDMVehicle): its action is decided once, at t == 0
          if (t == 0) generate_actions(v);
          idm_step(v);
        } else {
          // every v0 MDPVehicle has id 0 (controller.py:49): a neighbour follows actions[0] of the current joint action
          step_live(v, v == idx ? act[idx] : act[0]);
        }
      }
      // check_collision against the neighbours' stored points, then the obstacle (abstract.py:721-742)
      for (int k = 0; k < 4; k++) {
        const int o = nb[k];
        if (o < 0 || S.live(LCR, idx) != 0) continue;
        if (colliding(S.live(LX, idx), S.live(LY, idx), S.live(LH, idx), tx(t, o), ty(t, o), S.traj(t, 2, o),
                      kVehLength, kVehWidth)) {
          const double ev = S.live(LV, idx), ov = S.traj(t, 3, o);
          const double m = fabs(ov) < fabs(ev) ? ov : ev;  // min([speed, other speed], key=abs): first on ties
          S.live(LV, idx) = m;
          S.traj(t, 3, o) = m;
          S.live(LCR, idx) = 1;
          S.live(LCR, o) = 1;
        }
      }
      if (S.live(LCR, idx) == 0 && colliding(S.live(LX, idx), S.live(LY, idx), S.live(LH, idx), kObstX, kObstY, 0.0, 2.0, 2.0)) {
        const double ev = S.live(LV, idx);
        S.live(LV, idx) = fabs(ev) <= 0 ? ev : 0.0;
        S.live(LCR, idx) = 1;
      }
      if (S.live(LCR, idx) == 0) continue;
      // replacement (:151-176): every available action rolled t + 1 sub-steps from the original vehicle, first max room
      const double x0 = F(MM_F_X, idx), y0 = F(MM_F_Y, idx), h0 = F(MM_F_HEADING, idx), v0 = F(MM_F_SPEED, idx);
      const double ts0 = F(MM_F_TARGET_SPEED, idx);
      const int tl0 = B(MM_B_TARGET_LANE, idx);
      const bool cr0 = B(MM_B_CRASHED, idx) != 0;
      int best = -1;
      double best_room = 0;
      for (int c = 0; c < na; c++) {
        const int ca = avail[c];
        double x = x0, y = y0, h = h0, sp = v0, ts = ts0;
        int tl = tl0;
        double room_min = 0;
        for (int tt = 0; tt <= t; tt++) {  // check_safety_room (abstract.py:242-280)
          mdp_step(x, y, h, sp, ts, tl, cr0, ca, dt);
          double room = lane == MM_LANE_BC1 ? 420.0 - x : 100.0;
          if (ca == 0 || ca == 2) {
            const int sv[4] = {nb[0], nb[1], nb[2], nb[3]};
            for (int k = 0; k < 4; k++)
              if (sv[k] >= 0) {
                const double d = fabs(tx(tt, sv[k]) - x);
                if (d <= room) room = d;
              }
          } else {
            const int o = is_main(lane) ? nb[0] : nb[2];
            if (o >= 0) {
              const double d = tx(tt, o) - x;
              if (d <= room) room = d;
            }
          }
          if (tt == 0 || room < room_min) room_min = room;
        }
        if (best < 0 || room_min > best_room) { best = c; best_room = room_min; }
      }
      // the ego becomes the winning rollout (trajectory of t + 1 points); the first replacement rewrites the action
      reset_live(idx);
      for (int tt = 0; tt <= t; tt++) step_live(idx, avail[best]);
      if (first_change) { first_change = false; act[idx] = avail[best]; }
      for (int k = 0; k < 4; k++)
        if (nb[k] >= 0) S.live(LCR, nb[k]) = 0;
    }
  }
  for (int v = 0; v < N; v++) a.new_actions[b0 + v] = act[v];
  if (a.n_draws) a.n_draws[e] = nd;
}

}  // namespace sup
}  // namespace mm

static int32_t n_points_of(const MMConfig &c, int32_t n_step) {
  return (c.policy_frequency > 0 ? c.simulation_frequency / c.policy_frequency : 0) * n_step;
}
static uint64_t scratch_need(int32_t E, int32_t N, int32_t np) {
  return 8ull * (uint64_t)E * (uint64_t)N * (uint64_t)(mm::sup::kLive + mm::sup::kTraj * np);
}

extern "C" int32_t mm_supervise_scratch_bytes(int32_t E, int32_t N, int32_t n_step, int32_t sub_steps, uint64_t *bytes) {
  if (!bytes || E <= 0 || N <= 0 || N > MM_MAX_AGENTS || n_step < 1 || sub_steps < 1) return MM_ERR_INVALID_ARG;
  *bytes = scratch_need(E, N, sub_steps * n_step);
  return MM_OK;
}

extern "C" int32_t mm_supervise(MMHandle hd, int32_t kind, int32_t n_step, const int32_t *actions, const double *uniforms,
                                int32_t uniform_stride, void *scratch, uint64_t scratch_bytes, int32_t *new_actions,
                                int32_t *n_draws, MMStream stream) {
  if (!hd) return MM_ERR_INVALID_ARG;
  const MMHandleHead *h = mm_handle_head(hd);
  const MMConfig &c = h->cfg;
  const int32_t np = n_points_of(c, n_step);
  if (c.env_kind != MM_ENV_V0 || kind != MM_SUP_PRIORITY || n_step < 1 || np < 1 || !actions || !new_actions || !scratch ||
      ((uintptr_t)scratch & 7u) || (uniforms && uniform_stride < 9 * h->N) || scratch_bytes < scratch_need(h->E, h->N, np))
    return MM_ERR_INVALID_ARG;
  mm::sup::Args a;
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
  a.E = h->E; a.N = h->N; a.n_points = np;
  a.dt = 1.0 / c.simulation_frequency;
  a.headway_time = c.headway_time;
  const dim3 grid((unsigned)((h->E + 63) / 64));
  if (uniforms) hipLaunchKernelGGL(mm::sup::supervise_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(mm::sup::supervise_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

// mm_supervisor_dev.h -- device helpers shared by the two action-replacement supervisors (mm_supervisor.hip "priority",
// mm_supervisor_dmc.hip "dmc"; include/mm_supervisor.h): the lane acceptance of surrounding_vehicles, the integrators of
// mdp_controller.py / idm_controller.py, the IDM acceleration and the front-vehicle search of generate_actions, the
// collision test of abstract.py:744-755, the priority key of central_layer.py:32-65 and the Philox draw.  The arithmetic is
// the step kernel's (mm_device.h, include/mm_math.h).
#ifndef MM_SUPERVISOR_DEV_H
#define MM_SUPERVISOR_DEV_H

#include "mm_device.h"

namespace mm {
namespace sup {

constexpr uint32_t kDomain = 0x53555056u;  // Philox domain word of the supervisor's draws

// draw d of an env (include/mm_supervisor.h): u53 of Philox4x32-10 with counter (d, episode, steps, kDomain), key = seed
MM_DEV double philox_draw(int d, uint32_t episode, uint32_t steps, uint64_t seed) {
  uint32_t w[4];
  philox4x32((uint32_t)d, episode, steps, kDomain, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  return u53(w[0], w[1]);
}

// surrounding_vehicles (road.py:294-346): which lanes a query on lane `q` accepts
MM_DEV bool accepts(int q, int l) {
  switch (q) {
    case MM_LANE_AB0: return l == MM_LANE_AB0 || l == MM_LANE_BC0;
    case MM_LANE_BC0: return l == MM_LANE_AB0 || l == MM_LANE_BC0 || l == MM_LANE_CD0;
    case MM_LANE_CD0: return l == MM_LANE_BC0 || l == MM_LANE_CD0;
    case MM_LANE_JK0: return l == MM_LANE_JK0 || l == MM_LANE_KB0;
    case MM_LANE_KB0: return l == MM_LANE_JK0 || l == MM_LANE_KB0 || l == MM_LANE_BC1;
    default: return l == MM_LANE_KB0 || l == MM_LANE_BC1;  // bc1
  }
}
MM_DEV bool is_main(int l) { return l == MM_LANE_AB0 || l == MM_LANE_BC0 || l == MM_LANE_CD0; }

// mdp_controller.py:19-64 on a state held in registers; returns nothing, advances (x, y, h, v, ts, tl)
MM_DEV void mdp_step(double &x, double &y, double &h, double &v, double &ts, int &tl, bool crashed, int action, double dt) {
  if (lane_after_end(tl, x)) tl = next_lane(tl, x, y);  // follow_road :67-73
  if (action == 3) ts += 5;
  else if (action == 4) ts -= 5;
  else if (action == 2 || action == 0) {
    int cand = tl;  // np.clip(_id -/+ 1, ...): only road (b,c) has two lanes
    if (lane_road(tl) == 1) cand = action == 2 ? MM_LANE_BC1 : MM_LANE_BC0;
    if (lane_reachable(cand, x, y)) tl = cand;
  }
  double ht;
  steering_control(x, y, h, v, tl, ht);  // clipped to +-pi/3 already (:52 clips again: no-op)
  double acc = (1 / kTauA) * (ts - v);  // speed_control :107-115
  if (crashed) { ht = 0.0; acc = -1.0 * v; }  // clip_actions :118-127
  if (v > kMaxSpeed) { const double c = 1.0 * (kMaxSpeed - v); acc = acc <= c ? acc : c; }
  else if (v < -kMaxSpeed) { const double c = 1.0 * (kMaxSpeed - v); acc = acc >= c ? acc : c; }
  double sh, ch, sb, cb;
  mmm_sincos(h, &sh, &ch);
  mmm_slip_sincos(ht, &sb, &cb);  // beta = arctan(1/2 tan(delta))
  const double vx = v * mmm_cos_sum(sh, ch, sb, cb), vy = v * mmm_sin_sum(sh, ch, sb, cb);
  x = x + vx * dt;
  y = y + vy * dt;
  h = h + MM_DIVC(v * sb, 2.5) * dt;  // / (LENGTH / 2)
  v = v + acc * dt;
}

// idm_controller.py:41-56 for a vehicle that is not crashed: clip_actions (:230-239) writes into the action dict, which
// generate_actions left as vehicle.action, so the clipped acceleration persists (acc is updated)
MM_DEV void idm_move(double &x, double &y, double &h, double &sp, double steer, double &acc, double dt) {
  if (sp > kMaxSpeed) { const double c = 1.0 * (kMaxSpeed - sp); acc = acc <= c ? acc : c; }
  else if (sp < -kMaxSpeed) { const double c = 1.0 * (kMaxSpeed - sp); acc = acc >= c ? acc : c; }
  double s2, c2, sh, ch, sb, cb;
  mmm_sincos(steer, &s2, &c2);
  mmm_slip_sincos(1.0 / 2 * (s2 / c2), &sb, &cb);  // beta = arctan(1/2 tan(delta))
  mmm_sincos(h, &sh, &ch);
  const double vx = sp * mmm_cos_sum(sh, ch, sb, cb), vy = sp * mmm_sin_sum(sh, ch, sb, cb);
  x = x + vx * dt;
  y = y + vy * dt;
  h = h + MM_DIVC(sp * sb, 2.5) * dt;
  sp = sp + acc * dt;
}

// idm_controller.py:200-227 acceleration (IDM) of `ego` behind `front` (has_front false: none); lane = ego's lane
MM_DEV double idm_acc(int lane, double x, double h, double v, double ts, bool has_front, double fx, double fh, double fv) {
  const double target = not_zero(ts);
  const double q = fmax(v, 0) / target, q2 = q * q;
  double acc = 3.0 * (1 - q2 * q2);  // np.power(., 4) as (x^2)^2, as the step kernel
  if (has_front) {
    const double sx = lane_sx(lane);
    const double d = (fx - sx) - (x - sx);  // ego.lane_distance_to(front)
    double es, ec, fs, fc;
    mmm_sincos(h, &es, &ec);
    mmm_sincos(fh, &fs, &fc);
    const double dv = (v * ec - fv * fc) * ec + (v * es - fv * fs) * es;  // desired_gap :274-289, projected
    constexpr double den = 0x1.efbdeb14f4edap+2;  // 2 * np.sqrt(15.0)
    const double dstar = 10.0 + v * 1.5 + div_c(v * dv, den, 1.0 / den);
    const double g = dstar / not_zero(d);
    acc -= 3.0 * (g * g);
  }
  return acc;
}

// generate_actions (idm_controller.py:59-76) of HDV v on lane L at (x, y, h, sp): IDM behind the front vehicle of its own
// (original) lane, MOBIL, and two draws u1, u2 scaling steering and acceleration.  change_lane_policy returns the vehicle's
// lane in both of its branches: when lane != target lane directly (:99-111: the abort test `v is v.lane_index != ...` is
// always false), otherwise after MOBIL, which never accepts -- its "new" and "old" neighbours come from the same own-lane
// query (:137,144), so self_pred_a == self_a and the jerk is 0 < LANE_CHANGE_MIN_ACC_GAIN (an HDV has no route, :146).
// pose(u, ux, uy, uh, uv): the copy's vehicle u as it is now.  front: the front vehicle found (-1 none, nv the obstacle).
template <class Pose>
MM_DEV void hdv_generate(int v, int L, int nv, double x, double y, double h, double sp, double ts, double u1, double u2,
                         Pose pose, double &steer_out, double &acc_out, int &front) {
  // neighbour_vehicles (:242-271): road.vehicles + road.objects on the lane, margin 1
  double s, r;
  lane_local(L, x, y, s, r);
  bool hf = false;
  double sf = 0, fx = 0, fh = 0, fv = 0;
  front = -1;
  for (int u = 0; u <= nv; u++) {
    if (u == v) continue;
    const bool obst = u == nv;
    double ux = kObstX, uy = kObstY, uh = 0.0, uv = 0.0;
    if (!obst) pose(u, ux, uy, uh, uv);
    double su, ru;
    lane_local(L, ux, uy, su, ru);
    if (!(fabs(ru) <= kLaneWidth / 2 + 1 && -kVehLength <= su && su < lane_len(L) + kVehLength)) continue;
    if (s <= su && (!hf || su <= sf)) {
      sf = su; hf = true; front = u;
      fx = ux; fh = uh; fv = uv;
    }
  }
  const double steer = steering_control(x, y, h, sp, L);
  steer_out = clipd(steer * (u1 * 0.1 + 0.95), -kPi / 3, kPi / 3);
  const double acc = idm_acc(L, x, h, sp, ts, hf, fx, fh, fv);
  acc_out = clipd(acc * (u2 * 0.1 + 0.95), -6.0, 6.0);
}

// abstract.py:744-755 _is_colliding: norm > LENGTH pre-check, then the 0.9-scaled rectangles
MM_DEV bool colliding(double ex, double ey, double eh, double ox, double oy, double oh, double ol, double ow) {
  const double dx = ox - ex, dy = oy - ey;
  if ((dx * dx + dy * dy) > kU5) return false;
  return rects_intersect(ex, ey, eh, ox, oy, ol, ow, oh);
}

// the priority number of a controlled vehicle before its tie-breaking draw (central_layer.py:32-57, decentralised_dmc.py
// :89-114), on the ORIGINAL env: lane l, position (x, y), speed sp; lane_of(v) / x_of(v) over road.vehicles 0..nv-1
template <class LaneOf, class XOf>
MM_DEV double priority_number(int l, double x, double y, double sp, int nv, double headway_time, LaneOf lane_of, XOf x_of) {
  double p = 0;
  if (l == MM_LANE_BC1) {
    p = -0.5;
    const double dme = 420.0 - x;  // distance_to_merging_end (abstract.py:614-618): sum(ends[:3]) - x
    p = p - MM_DIVC(100.0 - dme, 100.0);
  }
  // _compute_headway_distance (abstract.py:620-635) on the original env
  double hd = 60;
  const int nl = next_lane(l, x, y);
  for (int v = 0; v < nv; v++) {
    const int lv = lane_of(v);
    const double xv = x_of(v);
    if (lv == l && xv > x) { const double d = xv - x; if (d < hd) hd = d; }
    if (l != MM_LANE_BC1 && lv == nl && xv > x) { const double d = xv - x; if (d < hd) hd = d; }
  }
  if (sp > 0) p = p + 0.5 * mmm_log(hd / (headway_time * sp));
  else p = p + 0;
  return p;
}

// _get_available_actions (abstract.py:219-240) of a vehicle on `lane` at (x, y) with speed index sidx, in the reference's
// list order: IDLE, LANE_LEFT, LANE_RIGHT, FASTER, SLOWER; returns the count
MM_DEV int available_actions(int lane, double x, double y, int sidx, int avail[5]) {
  int na = 0;
  avail[na++] = 1;
  if (lane == MM_LANE_BC1 && lane_reachable(MM_LANE_BC0, x, y)) avail[na++] = 0;
  if (lane == MM_LANE_BC0 && lane_reachable(MM_LANE_BC1, x, y)) avail[na++] = 2;
  if (sidx < 5 - 1) avail[na++] = 3;
  if (sidx > 0) avail[na++] = 4;
  return na;
}

}  // namespace sup
}  // namespace mm
#endif  // MM_SUPERVISOR_DEV_H

"""The pins of the four device kernels that run the damped least-squares iteration (csrc/vmv_robot_tu.inc: lm_start,
lm_accept, lm_step and constraint_project_lane's own loop): ik_batch, cartesian_multi, project_batch and the constraint round of
rrtc_multi_constrained, on inputs the other device tests already share.  compute() runs them through the public Python API
alone and returns, per call, the small integer outputs in clear and SHA-256 digests of the raw bytes of every float output.
tools/make_lm_golden.py writes that as tests/golden/lm_parent.json; tests/test_lm_pins_gpu.py holds a build to it bit for bit."""
import hashlib
import json
import os

import numpy as np

import cartesian_serial as C
import constraint_serial as S
import envs
import ik_serial as K

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_parent.json")
ROBOTS = K.ROBOTS
IK_TARGETS = 3  # x 32 seeds: 96 lanes, a full one-wave workgroup and a partial one
IK_SPOILED = (1, 7)  # (target, seed) of the seed row set non-finite
NAMES = ("upright", "plane", "box_cone")
NONFINITE_ROW = 5  # of constraint_serial.configs: spoiled in every projection
# rrtc_multi_constrained: test_rrtc_constrained_gpu.py's smallest table (its OTHERS rows), for every robot
RRTC = (("empty", 0, (1,), 0, 256), ("empty", 2, (-1,), 0, 256), ("cage", 0, (1, 2), 1000, 256), ("cage", 3, (4,), 2000, 256))
RRTC_ANGLE, RRTC_RANGE = 0.2, 0.5


def sha(a):
    return "sha256:" + hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def flags(a):
    return "".join("1" if x else "0" for x in np.asarray(a).reshape(-1))


def ints(a):
    return [int(x) for x in np.asarray(a).reshape(-1)]


def to_vamp(vamp, c):
    return vamp.EEConstraint(frame=c.frame, pos_lo=c.pos_lo, pos_hi=c.pos_hi, tool_axis=c.tool_axis, ref_axis=c.ref_axis, max_angle=c.max_angle)


def ik_calls(vamp, robot):
    mod = getattr(vamp, robot)
    targets = mod.eefk_batch(K.target_configs(robot)[:IK_TARGETS])
    seeds = np.ascontiguousarray(np.broadcast_to(K.halton32(robot, 32, K.SEED_SKIP)[None], (IK_TARGETS, 32, mod.dimension()))).copy()
    seeds[IK_SPOILED[0], IK_SPOILED[1], 0] = np.nan
    out = {}
    for name, kw in (("full", dict(halton_skip=K.SEED_SKIP, settings=vamp.IKSettings())),
                     ("position_only", dict(halton_skip=K.SEED_SKIP, settings=vamp.IKSettings(position_only=True))),
                     ("spoiled_seed", dict(seeds=seeds, settings=vamp.IKSettings()))):
        q, err, conv, its = mod.ik_batch(targets, **kw)
        out["ik_batch/" + name] = dict(converged=flags(conv), evaluations=ints(its), q=sha(q), err=sha(err))
    return out


def cartesian_calls(vamp, robot):
    mod, P = getattr(vamp, robot), vamp.planning
    starts, targets, _ = C.cases(robot)
    out = {}
    for name, s in (("full", P.CartesianSettings()), ("position_only", P.CartesianSettings(position_only=True)),
                    ("two_iterations", P.CartesianSettings(max_iterations=2))):
        paths = P.cartesian_multi(mod, starts, targets, None, s)
        out["cartesian_multi/" + name] = dict(status=[r.status for r in paths], segments=ints([r.segments for r in paths]),
                                              achieved=ints([r.achieved for r in paths]), evaluations=ints([r.evaluations for r in paths]),
                                              paths=sha(np.concatenate([r.path for r in paths])))
    return out


def antiparallel(vamp, robot, q):
    """-> (row, constraint): the first row of q whose tool axis z, as the device's own frame holds it, comes back bit for bit
    from the record's set-up of its negative as the reference axis; the row's axes are then antiparallel exactly (a x d = 0
    in fp32: both products of every component are the same two numbers).  (None, None) if no row of q is such a one."""
    F = getattr(vamp, robot).eefk_batch(q)
    for i in range(len(q)):
        a = F[i, :3, 2].astype(np.float64)
        c = S.Constraint(tool_axis=(0.0, 0.0, 1.0), ref_axis=tuple(-a), max_angle=0.1)
        if np.array_equal(S.record(c, S.Settings())["d"].astype(np.float32), (-a).astype(np.float32)):
            return i, c
    return None, None


def constraint_calls(vamp, robot):
    mod = getattr(vamp, robot)
    q = S.configs(robot)
    row, anti = antiparallel(vamp, robot, q)
    q = q.copy()
    q[NONFINITE_ROW, 1] = np.inf
    out = {}
    for name, c in S.cases(robot).items():
        for layout in ("shared", "per_lane"):
            records = to_vamp(vamp, c) if layout == "shared" else [to_vamp(vamp, c)] * S.N
            if layout == "per_lane" and row is not None:  # the antiparallel row rides in the per-lane layout, its own record
                records = list(records)
                records[row] = to_vamp(vamp, anti)
            got, res, conv, evals = mod.project_batch(q, records)
            out[f"project_batch/{name}/{layout}"] = dict(converged=flags(conv), evaluations=ints(evals), q=sha(got), res=sha(res),
                                                         antiparallel_row=-1 if row is None or layout == "shared" else int(row))
    return out


def rrtc_call(vamp, robot):
    mod, P = getattr(vamp, robot), vamp.planning
    constraint = vamp.EEConstraint.upright((0, 0, 1), RRTC_ANGLE)
    raw = S.configs(robot, 96)
    problems = []
    for kind, s, goals, skip, _ in RRTC:  # test_rrtc_constrained_gpu.Case's endpoints
        spec = envs.spec_for(kind, robot)
        env = envs.build_product_env(spec) if spec else None
        (rows,) = P.project_goals(mod, [raw], constraint, env)
        near = (rows[s] + np.float32(0.05) * S.ee_mask(robot)).astype(np.float32)
        (near,) = P.project_goals(mod, [near[None]], constraint, env)
        problems.append((env, rows[s], np.stack([near[0] if g < 0 else rows[g] for g in goals]), skip))
    got = P.rrtc_multi_constrained(mod, np.stack([p[1] for p in problems]), [p[2] for p in problems], [p[0] for p in problems], constraint,
                                   P.RRTCMultiSettings(range=RRTC_RANGE, max_iterations=1500, max_samples=RRTC[0][4]),
                                   skips=[p[3] for p in problems])
    paths = [np.asarray(g.path, np.float32).reshape(-1, mod.dimension()) for g in got]
    return {"rrtc_multi_constrained": dict(status=[str(g.status) for g in got], iterations=ints([g.iterations for g in got]),
                                           size=ints([list(g.size) for g in got]), waypoints=[len(p) for p in paths],
                                           goal_index=ints([g.goal_index for g in got]), band_refused=ints([g.band_refused for g in got]),
                                           endpoints=sha(np.concatenate([np.concatenate([p[1][None], p[2]]) for p in problems])),
                                           paths=sha(np.concatenate(paths)))}


def compute(vamp, robot):
    """-> {call: {field: clear integers / flags / digest}} for one robot"""
    return {**ik_calls(vamp, robot), **cartesian_calls(vamp, robot), **constraint_calls(vamp, robot), **rrtc_call(vamp, robot)}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def differences(want, got):
    """the fields of one robot's calls that differ, the clear-text ones first and element by element:
    'ik_batch/full evaluations: lane 17: 9, parent 8'"""
    clear, digests = [], []
    for call in sorted(set(want) | set(got)):
        w, g = want.get(call), got.get(call)
        if w is None or g is None:
            clear.append(f"{call}: {'not in the golden' if w is None else 'not computed'}")
            continue
        for field in sorted(set(w) | set(g)):
            a, b = w.get(field), g.get(field)
            if a == b:
                continue
            if isinstance(a, str) and a.startswith("sha256:"):
                digests.append(f"{call} {field}: {str(b)[:23]}..., parent {a[:23]}...")
            elif isinstance(a, (list, str)) and isinstance(b, type(a)) and len(a) == len(b):
                clear += [f"{call} {field}: lane {i}: {y}, parent {x}" for i, (x, y) in enumerate(zip(a, b)) if x != y]
            else:
                clear.append(f"{call} {field}: {b}, parent {a}")
    return clear + digests

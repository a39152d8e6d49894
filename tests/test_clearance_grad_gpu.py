"""<robot>.clearance_grad_batch / clearance_grad_batch_multi / planning.push_out on the device.

The gradient is checked against float64: the device's witness is taken as it is, the float64 distance of THAT fixed
witness is built as a function of q (tests/clearance_grad_ref.py: the generator's float64 tape, the distance forms of
tests/geom64.py, a heightfield's cell fixed as geom64.heightfield_cells gives it at q), and its central difference
(h = 1e-6) is compared with the device's fp32 gradient.  A case (configuration, value, joint) is left out only where the
fixed witness's own distance has a kink within h of q (clearance_grad_ref.kinks), at most 1 % per (robot, scene);
tests/test_clearance_grad.py holds the same seeds against that cap on the CPU.  The bound is
clearance_grad_ref.GRAD_BOUND; the figures behind it stand beside the constant.  Everything else is bit for bit:
values and witness against clearance_batch, batch independence, multi against single calls."""
import numpy as np
import pytest

import clearance_grad_ref as ref
import envs
import geom64
from test_clearance_gpu import BATCHES, KINDS, NONE, ROBOTS, contact_columns, halton, scene, self_pairs

pytestmark = pytest.mark.gpu

N_CONFIGS, SKIP = 257, 0  # partial waves, more than one tile of either size


def configurations(robot, n=N_CONFIGS, skip=SKIP):
    """the float32 Halton configurations of the float64 check (no device needed: test_clearance_grad.py reads them too)"""
    return ref.halton_q(ref.model(robot), n, skip).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_witness(oracle, robot, spec, q, witness):
    """the device's witness [n][4] as clearance_grad_ref.witness_quotients takes it"""
    tables, hfs, _ = contact_columns(spec)
    env_w = []
    for i, (s, kind, index, _) in enumerate(witness):
        if kind == NONE:
            env_w.append(None)
        elif kind < 5:
            env_w.append(dict(sphere=int(s), kind=int(kind), prim=np.asarray(tables[KINDS[kind]][index], np.float64), height=None))
        else:
            assert index == 0  # (geom64.heightfield_cells reads the first heightfield; these scenes hold one)
            centre, scale, xd, yd, data = hfs[0]
            cell = geom64.heightfield_cells(oracle, robot, list(spec), q[i])[0, s]
            idx = int(np.clip(np.rint(cell), 0, xd * yd - 1))
            inv_z = np.float32(1.0) / np.float32(scale[2])
            height = np.float64(inv_z) * np.float64(np.asarray(data, np.float32).reshape(-1)[idx]) + np.float64(np.float32(centre[2]))
            env_w.append(dict(sphere=int(s), kind=5, prim=None, height=float(height)))
    return env_w, np.where(witness[:, 3] == NONE, -1, witness[:, 3].astype(np.int64))


def check_gradient(vamp, oracle, robot, spec, q, label):
    """-> the device's (values, grad, witness) for q after holding grad against the float64 quotients of its witness"""
    mod = getattr(vamp, robot)
    env = envs.build_product_env(list(spec))
    values, grad, witness = mod.clearance_grad_batch(q, env, witness=True)
    n, dim = q.shape
    assert values.shape == (n, 2) and grad.shape == (n, 2, dim) and witness.shape == (n, 4)
    assert values.dtype == np.float32 and grad.dtype == np.float32 and witness.dtype == np.uint32
    env_w, self_w = device_witness(oracle, robot, spec, q, witness)
    pairs = self_pairs(vamp, robot)
    qe, qs = ref.witness_quotients(robot, q.astype(np.float64), env_w, self_w, pairs)
    left_out, worst = 0, []
    for half, quot in ((0, qe), (1, qs)):
        kink = ref.kinks(quot)
        dev = np.abs(grad[:, half].astype(np.float64) - quot[0])
        left_out += int(kink.sum())
        worst.append(float(dev[~kink].max()))
    print(f"{label}: n = {n}, {left_out} of {2 * q.size} cases left out at kinks, largest deviation env {worst[0]:.3e}, "
          f"self {worst[1]:.3e} per radian (bound {ref.GRAD_BOUND:.0e})")
    assert left_out <= ref.KINK_CAP * 2 * q.size, label
    assert max(worst) <= ref.GRAD_BOUND, label
    return values, grad, witness


# ---- the gradient against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["six", "many"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_gradient_matches_the_float64_difference_of_the_fixed_witness(vamp, oracle, robot, kind):
    q = configurations(robot)
    values, grad, witness = check_gradient(vamp, oracle, robot, scene(robot, kind), q, f"{robot} {kind}")
    assert (witness[:, 1] != NONE).all() and (witness[:, 3] != NONE).all()
    assert np.abs(grad).max() < 4.0  # a lever arm: no centre is further than 4 m from a joint axis


@pytest.mark.parametrize("kind", KINDS + ("heightfield",))
def test_each_kind_alone(vamp, oracle, kind):
    """every normal on its own: the scenes of test_clearance_gpu.test_each_kind_alone, where each kind is the witness"""
    q = halton(vamp, "panda", 65, 1000)
    values, grad, witness = check_gradient(vamp, oracle, "panda", scene("panda", kind), q, f"panda {kind} alone")
    assert (witness[:, 1] == (KINDS + ("heightfield",)).index(kind)).all()
    assert (np.abs(grad[:, 0]).max(axis=1) > 0).any()


def test_a_centre_inside_a_cuboid_has_env_gradient_zero(vamp):
    """the value is the flat -r there, so the gradient is 0: a box around the centre of the largest fine
    sphere - a sphere outside the box has d - r > -r >= -r_max, so the witness's centre is inside"""
    mod = vamp.panda
    q = halton(vamp, "panda", 3, 50)
    fk = mod.fk_batch(q)
    s = int(np.argmax(fk[0, :, 3]))
    box = envs.rot_cuboid(fk[0, s, :3] + np.array([0.01, -0.02, 0.015], np.float32), np.array([0.3, -0.2, 0.5]),
                          np.array([0.06, 0.06, 0.06]))
    env = envs.build_product_env([("cuboid", box)])
    values, grad, witness = mod.clearance_grad_batch(q, env, witness=True)
    assert witness[0, 1] == 3 and fk[0, witness[0, 0], 3] == fk[0, s, 3] and values[0, 0] == -fk[0, s, 3]
    c = fk[0, witness[0, 0], :3].astype(np.float64)[None]
    assert geom64.cuboid_clearance(c, np.zeros(1), np.asarray(box, np.float64)[None])[0, 0] == 0.0  # the centre is inside
    assert (grad[0, 0] == 0).all() and np.abs(grad[0, 1]).max() > 0
    assert np.array_equal(bits(grad[:, 1]), bits(mod.clearance_grad_batch(q, None)[1][:, 1]))


# ---- bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_values_and_witness_are_those_of_clearance_batch(vamp, robot):
    import torch

    mod = getattr(vamp, robot)
    env = envs.build_product_env(list(scene(robot, "six")))
    q = halton(vamp, robot, 257, 2000)
    want_v, want_w = mod.clearance_batch(q, env, witness=True)
    values, grad, witness = mod.clearance_grad_batch(q, env, witness=True)
    assert np.array_equal(bits(values), bits(want_v)) and np.array_equal(witness, want_w)
    v2, g2 = mod.clearance_grad_batch(q, env)  # without a caller's witness buffer: the call's own scratch
    assert np.array_equal(bits(v2), bits(want_v)) and np.array_equal(bits(g2), bits(grad))
    # the device entry points (torch CUDA tensors in and out) agree with the host ones bit for bit
    qt = torch.from_numpy(q).cuda()
    vt, gt = mod.clearance_grad_batch(qt, env)
    assert np.array_equal(bits(vt.cpu().numpy()), bits(want_v)) and np.array_equal(bits(gt.cpu().numpy()), bits(grad))
    vt, gt, wt = mod.clearance_grad_batch(qt, env, witness=True)
    assert np.array_equal(bits(gt.cpu().numpy()), bits(grad)) and np.array_equal(wt.cpu().numpy().view(np.uint32), want_w)
    # one configuration
    (e, s), g = mod.clearance_grad(q[5], env)
    assert np.array_equal(np.array([e, s], np.float32), want_v[5]) and np.array_equal(bits(g), bits(grad[5]))


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_configuration_does_not_depend_on_its_batch(vamp, robot):
    mod = getattr(vamp, robot)
    env = envs.build_product_env(list(scene(robot, "six")))
    q = halton(vamp, robot, 257, 5000)
    probe = q[17].copy()
    alone = mod.clearance_grad_batch(probe[None, :], env)[1]
    for n in BATCHES:  # 1, 63, 64, 65, 257
        for at in sorted({0, n // 2, n - 1}):
            batch = q[:n].copy()
            batch[at] = probe
            assert np.array_equal(bits(mod.clearance_grad_batch(batch, env)[1][at]), bits(alone[0])), (n, at)


@pytest.mark.parametrize("robot", ROBOTS)
def test_multi_equals_single_calls_bit_for_bit(vamp, robot):
    import torch

    mod = getattr(vamp, robot)
    scenes = [envs.build_product_env(list(scene(robot, k))) for k in ("six", "many", "mixed")]
    counts = [100, 0, 93]  # ragged: more than one tile each, an empty segment, no multiple of a tile (64 or 32)
    q = halton(vamp, robot, sum(counts), 9000)
    values, grad, witness = mod.clearance_grad_batch_multi(q, scenes, counts, witness=True)
    assert values.shape == (193, 2) and grad.shape == (193, 2, q.shape[1]) and witness.shape == (193, 4)
    lo = 0
    for e, c in zip(scenes, counts):
        if c:
            v, g, w = mod.clearance_grad_batch(q[lo:lo + c], e, witness=True)
            assert np.array_equal(bits(values[lo:lo + c]), bits(v)) and np.array_equal(bits(grad[lo:lo + c]), bits(g))
            assert np.array_equal(witness[lo:lo + c], w)
        lo += c
    v2, g2 = mod.clearance_grad_batch_multi(q, scenes, counts)  # the call's own witness scratch
    assert np.array_equal(bits(v2), bits(values)) and np.array_equal(bits(g2), bits(grad))
    vt, gt = mod.clearance_grad_batch_multi(torch.from_numpy(q).cuda(), scenes, counts)
    assert np.array_equal(bits(vt.cpu().numpy()), bits(values)) and np.array_equal(bits(gt.cpu().numpy()), bits(grad))
    # a None among the environments is the empty environment
    v3, g3 = mod.clearance_grad_batch_multi(q[:40], [None, scenes[0]], [7, 33])
    assert (v3[:7, 0] == np.inf).all() and (g3[:7, 0] == 0).all()
    assert np.array_equal(bits(g3[7:]), bits(mod.clearance_grad_batch(q[7:40], scenes[0])[1]))


@pytest.mark.parametrize("robot", ROBOTS)
def test_without_an_environment_and_in_an_empty_one(vamp, robot):
    mod = getattr(vamp, robot)
    q = halton(vamp, robot, 70, 300)
    v_none, g_none = mod.clearance_grad_batch(q, None)
    v_empty, g_empty = mod.clearance_grad_batch(q, vamp.Environment())
    v_six, g_six = mod.clearance_grad_batch(q, envs.build_product_env(list(scene(robot, "six"))))
    for v, g in ((v_none, g_none), (v_empty, g_empty)):
        assert (v[:, 0] == np.inf).all() and (bits(g[:, 0]) == 0).all()  # zeros, +0
    assert np.array_equal(bits(g_none), bits(g_empty))
    assert np.array_equal(bits(g_six[:, 1]), bits(g_none[:, 1]))  # the self gradient does not depend on the environment
    assert np.abs(g_none[:, 1]).max() > 0 and np.abs(g_six[:, 0]).max() > 0


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_non_finite_joint_gives_nan_and_leaves_its_neighbours_alone(vamp, robot):
    mod = getattr(vamp, robot)
    env = envs.build_product_env(list(scene(robot, "six")))
    q = halton(vamp, robot, 130, 700)
    clean = mod.clearance_grad_batch(q, env)[1]
    assert np.isfinite(clean).all()
    bad = q.copy()
    rows = [0, 5, 63, 64, 129]
    for j, i in enumerate(rows):
        bad[i, j % q.shape[1]] = (np.nan, np.inf, -np.inf)[j % 3]
    others = np.setdiff1d(np.arange(130), rows)
    v, g = mod.clearance_grad_batch(bad, env)
    assert np.isnan(v[rows]).all() and np.isnan(g[rows]).all()
    assert np.array_equal(bits(g[others]), bits(clean[others]))
    v2, g2 = mod.clearance_grad_batch_multi(bad, [env, None], [100, 30])
    assert np.isnan(g2[rows]).all() and np.array_equal(bits(g2[:100][others[others < 100]]), bits(clean[others[others < 100]]))


# ---- push_out ------------------------------------------------------------------------------------------------------------
def test_push_out_moves_a_grazing_configuration_out_of_contact(vamp):
    """the Panda at the cage example's start, one sphere obstacle under its last fine sphere (a fingertip), 5 mm deep; the
    float64 tape says every other sphere is 17 mm or more from that obstacle and the self clearance is 15 mm"""
    from oracle_lib import CAGE_START
    from vamp_mvt_amd.planning import push_out

    mod = vamp.panda
    q0 = np.asarray(CAGE_START, np.float32)
    fk = mod.fk_batch(q0[None, :])[0]
    s, radius = len(fk) - 1, np.float32(0.05)
    centre = fk[s, :3].astype(np.float64) - np.array([0.0, 0.0, 1.0]) * (float(fk[s, 3]) + float(radius) - 0.005)
    env = envs.build_product_env([("sphere", np.array([*centre, radius], np.float32))])
    q = np.concatenate([q0[None, :], halton(vamp, "panda", 63, 400)])
    before, witness = mod.clearance_batch(q, env, witness=True)
    assert witness[0, 0] == s and abs(float(before[0, 0]) + 0.005) < 1e-5 and before[0, 1] > 0.01
    out = push_out(mod, q, env, margin=0.01, max_steps=32, max_step=0.05)
    assert out.configurations.shape == q.shape and out.clearances.shape == (64, 2) and 1 <= out.calls <= 33
    with np.errstate(invalid="ignore"):
        assert (out.clearances.min(axis=1) >= before.min(axis=1)).all()  # never worse than the input
    assert np.array_equal(bits(out.clearances), bits(mod.clearance_batch(out.configurations, env)))
    assert np.array_equal(out.reached, out.clearances.min(axis=1) >= np.float32(0.01))
    assert out.reached[0] and (out.configurations[0] != q0).any()
    lower, upper = mod.lower_bounds(), mod.upper_bounds()
    assert (out.configurations >= lower).all() and (out.configurations <= upper).all()
    print(f"push_out: {int(out.reached.sum())} of 64 reached the margin in {out.calls} calls; the constructed one moved "
          f"{float(np.abs(out.configurations[0] - q0).max()):.4f} rad to env {float(out.clearances[0, 0]):.5f} m")

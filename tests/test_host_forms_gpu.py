"""The host-buffer forms of the batched calls (numpy in) against their device forms (torch CUDA tensors in), bit for bit,
and the per-thread staging arena they share: across its keep limit, across vmv_release_staging(), and from two threads.
The device forms take the caller's device memory as it is and never touch the arena: they are the independent side."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import envs

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # one validity word, the word boundary, a partial last word
KEEP_BYTES = 64 << 20         # kStagingKeepBytes (vmv_api.hip)


@functools.lru_cache(maxsize=None)
def scenes(robot):
    return tuple(envs.build_product_env(envs.spec_for(kind, robot)) for kind in ("mixed", "cage"))


def configurations(robot, n, seed):
    lo, hi = np.asarray(robot.lower_bounds(), np.float32), np.asarray(robot.upper_bounds(), np.float32)
    return (lo + (hi - lo) * np.random.default_rng(seed).random((n, robot.dimension()), dtype=np.float32)).astype(np.float32)


def same(host, device):
    """bit for bit, NaNs included; a tuple element by element; the torch witness is int32"""
    if isinstance(host, tuple):
        assert isinstance(device, tuple) and len(host) == len(device)
        return all(same(h, d) for h, d in zip(host, device))
    d = device.cpu().numpy() if hasattr(device, "cpu") else device
    return host.shape == d.shape and host.dtype.itemsize == d.dtype.itemsize and host.tobytes() == d.tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["panda", "baxter"])
def test_host_forms_equal_device_forms(vamp, name, n):
    import torch

    robot = getattr(vamp, name)
    env, other = scenes(name)
    a = configurations(robot, n, 5)
    b = (a + np.random.default_rng(6).normal(0, 0.2, a.shape)).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    pair, counts = [env, other], [n // 3, n - n // 3]
    assert same(robot.validate_batch(a, env), robot.validate_batch(ta, env))
    assert same(robot.validate_motion_batch(a, b, env), robot.validate_motion_batch(ta, tb, env))
    assert same(robot.validate_batch_multi(a, pair, counts), robot.validate_batch_multi(ta, pair, counts))
    assert same(robot.validate_motion_batch_multi(a, b, pair, counts), robot.validate_motion_batch_multi(ta, tb, pair, counts))
    assert same(robot.fk_batch(a), robot.fk_batch(ta))
    assert same(robot.eefk_batch(a), robot.eefk_batch(ta))
    for witness in (False, True):
        for e in (env, None):
            assert same(robot.clearance_batch(a, e, witness=witness), robot.clearance_batch(ta, e, witness=witness))
            assert same(robot.clearance_grad_batch(a, e, witness=witness), robot.clearance_grad_batch(ta, e, witness=witness))
        assert same(robot.clearance_batch_multi(a, pair, counts, witness=witness),
                    robot.clearance_batch_multi(ta, pair, counts, witness=witness))
        assert same(robot.clearance_grad_batch_multi(a, pair, counts, witness=witness),
                    robot.clearance_grad_batch_multi(ta, pair, counts, witness=witness))
    spheres = robot.fk_batch(a).reshape(-1, 4)[:n].copy()  # free spheres where the robot's are: some hit, some do not
    ts, hits = torch.from_numpy(spheres).cuda(), torch.zeros(n, dtype=torch.uint8, device="cuda")
    vamp.check(vamp.lib.vmv_spheres_in_collision_batch(env.handle(), ctypes.c_void_p(ts.data_ptr()), n,
                                                       ctypes.c_void_p(hits.data_ptr()),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "vmv_spheres_in_collision_batch")
    assert same(env.spheres_in_collision(spheres), hits.bool())


def small_calls(vamp, q):
    """host calls of five different region layouts -> their results"""
    robot, env = vamp.panda, scenes("panda")[0]
    return (robot.fk_batch(q[:1]), robot.eefk_batch(q[:65]), env.spheres_in_collision(robot.fk_batch(q[:1])[0]),
            robot.validate_batch(q[:257], env), robot.clearance_batch(q[:63], env, witness=True))


def test_the_arena_across_its_keep_limit(vamp):
    robot = vamp.panda
    n = KEEP_BYTES // (robot.n_spheres() * 16 + robot.dimension() * 4) + 1024  # staged bytes of fk_batch: above the limit
    assert n * (robot.n_spheres() * 16 + robot.dimension() * 4) > KEEP_BYTES
    q = configurations(robot, n, 7)
    assert vamp.lib.vmv_release_staging() == 0
    first = small_calls(vamp, q)  # each made first in a fresh sequence
    assert vamp.lib.vmv_release_staging() == 0
    one = robot.fk_batch(q[:1])                 # a small arena
    large = robot.fk_batch(q)                   # grows past the keep limit, trimmed on the way out
    assert same(one, large[:1]) and same(first[0], large[:1])
    spot = np.random.default_rng(8).integers(0, n, 64)
    assert same(robot.fk_batch(q[spot]), large[spot])  # (the large call's rows, not only its first)
    assert same(small_calls(vamp, q), first)    # grows again; five layouts share it
    assert vamp.lib.vmv_release_staging() == 0
    assert same(small_calls(vamp, q), first)


def test_two_threads_have_an_arena_each(vamp):
    robot, env = vamp.panda, scenes("panda")[0]
    env.handle()  # finalized up front: the threads share the handle, not its construction
    q = configurations(robot, 257, 9)
    b = (q + np.float32(0.1)).astype(np.float32)
    kinds = (lambda m: robot.validate_batch(q[:m], env), lambda m: robot.fk_batch(q[:m]),
             lambda m: robot.clearance_batch(q[:m], env, witness=True), lambda m: robot.validate_motion_batch(q[:m], b[:m], env))

    def calls(shift):  # 20 calls of alternating kinds and sizes
        return [kinds[(i + shift) % 4]((1, 257)[(i // 2 + shift) % 2]) for i in range(20)]

    want = [calls(0), calls(1)]
    got, errors = [None, None], []

    def work(t):
        try:
            got[t] = calls(t)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in range(2):
        assert all(same(w, g) for w, g in zip(want[t], got[t]))

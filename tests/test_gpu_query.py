"""rtx_query on the GPU (query_kernel, csrc/hip/rtx_query.h) against the CPU
restatement's query_batch: closest hit and ordered all-hits lists, bit-exact
ids and t.  Scenes, counts, rays and seeds are test_traverse_host's — the
smallest that still reach mesh BVHs, cones, overlapping spheres and the
d[a] == 0 slab skip.  This is the traversal's on-device unit test: no shading,
no wavefront machinery around it."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import cli_opts, scene_path
from test_traverse_host import SCENES, _rays

pytestmark = pytest.mark.gpu

IDS = [s[0] for s in SCENES]


@functools.lru_cache(maxsize=None)
def _scene(pkg, scene):
    host = pkg.HostScene(scene_path(scene))
    return host, pkg.DeviceScene(host, 0)


@functools.lru_cache(maxsize=None)
def _case(pkg, orc, scene, n, seed, mode, kmax):
    """(device scene, rays, the restatement's answer): computed once, shared, read-only."""
    host, dev = _scene(pkg, scene)
    P, D = _rays(host, n, seed)
    ref = orc.query_batch(pkg, scene_path(scene), P, D, mode, kmax)
    for a in (P, D) + tuple(ref):
        a.setflags(write=False)
    return dev, P, D, ref


@pytest.mark.parametrize("scene,n", SCENES, ids=IDS)
def test_closest_parity(pkg, orc, scene, n):
    dev, P, D, (rt, ro, rf, rnh) = _case(pkg, orc, scene, n, 7, 0, 1)
    t, o, f, nh = dev.query(P, D, "closest")
    assert t.shape == (n, 1) and o.shape == (n, 1) and f.shape == (n, 1) and nh.shape == (n,)
    hit = rnh > 0
    assert np.array_equal(nh > 0, hit)
    assert np.array_equal(nh, hit.astype(np.int32))
    assert np.array_equal(o[:, 0], ro[:, 0])
    assert np.array_equal(f[:, 0], rf[:, 0])
    assert np.array_equal(t[hit, 0], rt[hit, 0]), "closest t not bit-exact"
    assert (t[~hit, 0] == 0.0).all()
    assert hit.mean() > 0.05


@pytest.mark.parametrize("scene,n", SCENES, ids=IDS)
def test_all_parity_kmax16(pkg, orc, scene, n):
    dev, P, D, (rt, ro, rf, rnh) = _case(pkg, orc, scene, n, 11, 1, 16)
    assert (rnh <= 16).all()  # std::sort stays in its stable range: no ray is excluded
    t, o, f, nh = dev.query(P, D, "all", 16)
    assert np.array_equal(nh, rnh)
    assert np.array_equal(o, ro)
    assert np.array_equal(f, rf)
    assert np.array_equal(t, rt)
    assert (rnh > 1).mean() > 0.05


@pytest.mark.parametrize("scene,n", [SCENES[1], SCENES[4]], ids=[IDS[1], IDS[4]])
def test_truncation_kmax4(pkg, orc, scene, n):
    dev, P, D, (rt, ro, rf, rnh) = _case(pkg, orc, scene, n, 11, 1, 16)
    assert (rnh <= 16).all()
    t, o, f, nh = dev.query(P, D, "all", 4)
    assert np.array_equal(nh, np.minimum(rnh, 4))
    assert np.array_equal(o, ro[:, :4])
    assert np.array_equal(f, rf[:, :4])
    assert np.array_equal(t, rt[:, :4])
    assert (rnh > 4).any()  # a list is actually cut


GUARD = 64
SENT_T, SENT_I = -7.5, -77


def _guarded_query(pkg, dev, P, D, mode, kmax):
    """rtx_query into sentinel-filled arrays with GUARD extra entries after
    the n * kmax (n) the call may write; returns the arrays whole."""
    lib = pkg.hip_lib()
    n = P.shape[0]
    t = np.full(n * kmax + GUARD, SENT_T, np.float64)
    o = np.full(n * kmax + GUARD, SENT_I, np.int32)
    f = np.full(n * kmax + GUARD, SENT_I, np.int32)
    nh = np.full(n + GUARD, SENT_I, np.int32)
    Pc = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    Dc = np.ascontiguousarray(D, np.float64).reshape(-1, 3)
    rc = lib.rtx_query(dev._s, mode, n, Pc.ctypes.data, Dc.ctypes.data, kmax, t.ctypes.data, o.ctypes.data,
                       f.ctypes.data, nh.ctypes.data, 0, None)
    assert rc == 0, lib.rtx_last_error()
    return t, o, f, nh


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 193])
def test_batch_edges(pkg, orc, n):
    scene, nmax = SCENES[0]
    dev, Pa, Da, (rta, roa, rfa, rnha) = _case(pkg, orc, scene, nmax, 11, 1, 16)
    _, _, _, (cta, coa, cfa, cnha) = _case(pkg, orc, scene, nmax, 11, 0, 1)
    # a stride over the ray set, so every n mixes camera, interior and axis-aligned rays
    idx = (np.arange(n) * (nmax // 193)) % nmax
    P, D = Pa[idx], Da[idx]
    for mode, kmax, (rt, ro, rf, rnh) in ((0, 1, (cta, coa, cfa, cnha)), (1, 16, (rta, roa, rfa, rnha))):
        t, o, f, nh = _guarded_query(pkg, dev, P, D, mode, kmax)
        m = n * kmax
        assert (t[m:] == SENT_T).all() and (o[m:] == SENT_I).all() and (f[m:] == SENT_I).all()
        assert (nh[n:] == SENT_I).all()
        assert np.array_equal(nh[:n], rnh[idx])
        assert np.array_equal(o[:m].reshape(n, kmax), ro[idx])
        assert np.array_equal(f[:m].reshape(n, kmax), rf[idx])
        used = np.arange(kmax)[None, :] < rnh[idx][:, None]
        assert np.array_equal(t[:m].reshape(n, kmax)[used], rt[idx][used])
        assert (t[:m].reshape(n, kmax)[~used] == 0.0).all()


def test_short_stacks(pkg, orc):
    """RTX_TEST_LDS_STACK=2: two stack entries per lane in LDS, the rest in
    the overflow columns in HBM — same answers, bit for bit."""
    scene, n = SCENES[5]
    assert scene == "trimesh2.ray" and n == 900
    dev, P, D, _ = _case(pkg, orc, scene, n, 11, 1, 16)
    base_c = dev.query(P, D, "closest")
    base_a = dev.query(P, D, "all", 16)
    saved = os.environ.get("RTX_TEST_LDS_STACK")
    os.environ["RTX_TEST_LDS_STACK"] = "2"
    try:
        short_c = dev.query(P, D, "closest")
        short_a = dev.query(P, D, "all", 16)
    finally:
        if saved is None:
            os.environ.pop("RTX_TEST_LDS_STACK", None)
        else:
            os.environ["RTX_TEST_LDS_STACK"] = saved
    for a, b in zip(base_c + base_a, short_c + short_a):
        assert np.array_equal(a, b)
    assert (base_a[3] > 1).any() and (base_c[3] > 0).any()


def _torch_child():
    """The body of test_device_pointers_on_a_stream, in a process of its own:
    torch's HIP runtime must initialise before the library's (bench.py's
    order); in the test process the library's already has."""
    import torch

    torch.cuda.set_device(0)
    cu = torch.device("cuda:0")
    torch.zeros(1, device=cu)
    from conftest import load_package

    pkg = load_package()
    scene, n = SCENES[4]
    host = pkg.HostScene(scene_path(scene))
    dev = pkg.DeviceScene(host, 0)
    P, D = _rays(host, n, 11)
    host_c = dev.query(P, D, "closest")
    host_a = dev.query(P, D, "all", 16)
    s = torch.cuda.Stream(device=cu)
    assert s.cuda_stream != torch.cuda.default_stream(cu).cuda_stream
    with torch.cuda.stream(s):
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(cu)
        dD = torch.from_numpy(np.ascontiguousarray(D)).to(cu)
        outs = []
        for mode, k in (("closest", 1), ("all", 16)):
            t = torch.full((n, k), SENT_T, dtype=torch.float64, device=cu)
            o = torch.full((n, k), SENT_I, dtype=torch.int32, device=cu)
            f = torch.full((n, k), SENT_I, dtype=torch.int32, device=cu)
            nh = torch.full((n,), SENT_I, dtype=torch.int32, device=cu)
            dev.query_device(n, dP.data_ptr(), dD.data_ptr(), mode, k, t.data_ptr(), o.data_ptr(), f.data_ptr(),
                             nh.data_ptr(), stream=s.cuda_stream)
            outs.append((t, o, f, nh))
    s.synchronize()
    for host_out, got in zip((host_c, host_a), outs):
        for a, b in zip(host_out, got):
            assert np.array_equal(a, b.cpu().numpy())
    assert (host_a[3] > 1).any() and (host_c[3] > 0).any()
    dev.close()
    print("torch-child ok")


def test_device_pointers_on_a_stream():
    """Torch tensors on the device, a non-default torch stream: the same
    answers as the host-pointer call.  (A child process: see _torch_child.)"""
    if importlib.util.find_spec("torch") is None:  # (not imported here: the child's runtime order)
        pytest.skip("torch is not installed")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_no_cross_talk_with_rendering(pkg, orc):
    scene, n = SCENES[1]
    assert scene == "spheres_overlap.ray"
    opts = cli_opts(pkg, "-w 32 -r 5 -O r -A 2")
    host = pkg.HostScene(scene_path(scene))
    P, D = _rays(host, n, 11)

    # the reference sequence: two renders, no query
    dev0 = pkg.DeviceScene(host, 0)
    dev0.kernel_time()
    r0 = dev0.render(opts)
    _, launches0a = dev0.kernel_time()
    dev0.render(opts)
    _, launches0b = dev0.kernel_time()
    dev0.close()

    dev = pkg.DeviceScene(host, 0)
    dev.kernel_time()
    r1 = dev.render(opts)
    _, la = dev.kernel_time()
    q1 = dev.query(P, D, "all", 16)
    _, lq = dev.kernel_time()
    r2 = dev.render(opts)
    _, lb = dev.kernel_time()
    q2 = dev.query(P, D, "all", 16)
    c2 = dev.query(P, D, "closest")
    dev.close()
    assert lq == 0  # a query counts no render launch
    assert (la, lb) == (launches0a, launches0b)
    assert r1["rgb8"].tobytes() == r2["rgb8"].tobytes() == r0["rgb8"].tobytes()
    assert r1["rgb"].tobytes() == r2["rgb"].tobytes() == r0["rgb"].tobytes()
    for a, b in zip(q1, q2):
        assert np.array_equal(a, b)
    rt, ro, rf, rnh = orc.query_batch(pkg, scene_path(scene), P, D, 1, 16)
    assert np.array_equal(q1[3], rnh) and np.array_equal(q1[1], ro) and np.array_equal(q1[0], rt)
    assert np.array_equal(c2[1][:, 0], ro[:, 0])  # the closest hit is the list's first entry


def test_invalid_arguments_on_a_live_scene(pkg, orc):
    scene, n = SCENES[0]
    dev, P, D, (rt, ro, rf, rnh) = _case(pkg, orc, scene, n, 7, 0, 1)
    lib = pkg.hip_lib()
    Pc, Dc = np.ascontiguousarray(P), np.ascontiguousarray(D)
    nh = np.full(n, SENT_I, np.int32)

    def call(mode, cnt, p, d, kmax):
        return lib.rtx_query(dev._s, mode, cnt, p, d, kmax, None, None, None, nh.ctypes.data, 0, None)

    INV, CAP = pkg.RTX_ERR_INVALID, pkg.RTX_ERR_CAPACITY
    assert call(2, n, Pc.ctypes.data, Dc.ctypes.data, 1) == INV
    assert call(0, -1, Pc.ctypes.data, Dc.ctypes.data, 1) == INV
    assert call(1, n, Pc.ctypes.data, Dc.ctypes.data, 0) == INV
    assert call(0, n, Pc.ctypes.data, Dc.ctypes.data, 2) == INV
    assert call(0, n, None, Dc.ctypes.data, 1) == INV
    assert call(1, n, Pc.ctypes.data, None, 16) == INV
    assert call(1, n, Pc.ctypes.data, Dc.ctypes.data, pkg.RTX_QUERY_KMAX + 1) == CAP
    assert b"rtx_query" in lib.rtx_last_error()
    assert (nh == SENT_I).all()  # no failed call wrote anything
    assert call(1, 0, None, None, 16) == pkg.RTX_OK  # n == 0: nothing to do
    assert (nh == SENT_I).all()
    with pytest.raises(pkg.RtxError):
        dev.query(P, D, "all", 0)
    # and the scene still answers
    t, o, f, nh2 = dev.query(P, D, "closest")
    assert np.array_equal(o, ro) and np.array_equal(nh2, rnh)
    hit = rnh > 0
    assert np.array_equal(t[hit], rt[hit])


if __name__ == "__main__":
    if sys.argv[1:] == ["--torch-child"]:
        _torch_child()

"""CPU-side checks of the trajectory -> GP dataset packing (ABI 13):
rcbf_traj_pack_gp_f64 / rcbf_traj_pack_gp_scratch_bytes exist and reject bad
arguments before any launch; their three kernels, as they stand in
librcbf_hip.so, use no scratch and spill nothing;
DynamicsModel.trajectory_rows / append_trajectory check their arguments before
the library is loaded; and _append_rows and the three refit modes reproduce the
reference's row-by-row ring, counter and fit points (dynamics.py:263-290,
restated as in tests/test_gp_host.py).  None of it needs a GPU."""
import ctypes
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from test_abi_cpu import ROOT

E_BAD_SHAPE, E_NULL = 1002, 1003
LIB = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_hip.so")


def test_symbols_and_abi_version():
    from rcbf_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rcbf_traj_pack_gp_f64") and hasattr(lib, "rcbf_traj_pack_gp_scratch_bytes")
    assert lib.rcbf_abi_version() == 13 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    assert re.search(r"#define\s+RCBF_ABI_VERSION\s+13\b", hdr)
    for name in ("rcbf_traj_pack_gp_f64", "rcbf_traj_pack_gp_scratch_bytes"):
        assert re.search(r"^int(64_t)?\s+%s\s*\(" % name, hdr, re.M), name
    assert "main.py:110-113" in hdr and "dynamics.py:263-303" in hdr


def test_scratch_bytes_is_a_count_per_step_and_wave_plus_the_total():
    from rcbf_amd import _lib
    lib = _lib.load()
    for B, K in ((1, 1), (64, 5), (65, 5), (130, 7), (65536, 20), (64, 1000)):
        assert lib.rcbf_traj_pack_gp_scratch_bytes(B, K) == 8 * ((B + 63) // 64 * K + 1)
    assert lib.rcbf_traj_pack_gp_scratch_bytes(1 << 31, 1000) == 8 * ((1 << 25) * 1000 + 1)  # past 2^32 bytes
    assert lib.rcbf_traj_pack_gp_scratch_bytes(-1, 5) == 0 == lib.rcbf_traj_pack_gp_scratch_bytes(5, 0)


def test_pack_gp_rejects_bad_arguments_without_a_gpu():
    from rcbf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # 16-byte aligned host memory: never dereferenced, no launch is reached

    def call(state=p, dist=p, count=p, scratch=p, B=4, K=2, P=4, n_o=10, n_u=1, obs0=p, step0=p, obs=p, term=p, u=p,
             done=p, auto_reset=1, every=2, keep_last=8):
        return lib.rcbf_traj_pack_gp_f64(state, dist, count, scratch, B, K, P, n_o, n_u, obs0, step0, obs, term, u,
                                         done, 0.02, auto_reset, every, keep_last, None)

    assert call(B=0) == 0  # an empty batch is a no-op
    assert call(B=0, state=None, term=None) == 0
    for kw in ({"P": 3}, {"K": 0}, {"K": -1}, {"B": -1}, {"every": 0}, {"every": -2}, {"keep_last": 0},
               {"keep_last": -1}, {"n_o": 9}, {"n_o": 7, "n_u": 1}, {"n_o": 10, "n_u": 2}):
        assert call(**kw) == E_BAD_SHAPE, kw
    for f in ("state", "dist", "count", "scratch", "obs0", "step0", "obs", "u", "done"):
        assert call(**{f: None}) == E_NULL, f
    # term_obs may be missing only without auto_reset: there is no warn-and-continue mode
    assert call(term=None) == E_NULL
    assert call(term=None, auto_reset=0, B=0) == 0
    # cars rows are read as 8-byte pairs; the outputs and the scratch hold 8-byte values
    odd = ctypes.c_void_p(p.value + 4)
    for f in ("obs0", "obs", "term", "state", "dist", "count", "scratch"):
        assert call(**{f: odd}) == E_BAD_SHAPE, f


def _gfx950_code_objects(path):
    """The gfx950 code objects in the library's offload bundles (one bundle per
    translation unit: magic, entry count, then (offset, size, triple) each)."""
    data = open(path, "rb").read()
    magic, out, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := data.find(magic, at)) >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(magic))
        q = at + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                out.append(data[at + off:at + off + size])
        at += len(magic)
    return out


def test_pack_gp_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    import yaml
    found = {}
    for k, blob in enumerate(_gfx950_code_objects(LIB)):
        if b"k_traj_pack_gp" not in blob:
            continue
        co = tmp_path / f"co{k}.elf"
        co.write_bytes(blob)
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(co)], check=True,
                             capture_output=True, text=True).stdout
        m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
        assert m, "no AMDGPU metadata"
        for kern in yaml.safe_load(m.group(1))["amdhsa.kernels"]:
            if re.search(r"k_traj_gp_count|k_traj_gp_scan|k_traj_pack_gp", kern[".name"]):
                found[kern[".name"]] = kern
    assert len(found) == 4, sorted(found)  # count, scan, pack x {cars, unicycle}
    for name, kern in found.items():
        assert kern[".private_segment_fixed_size"] == 0, name
        assert kern[".sgpr_spill_count"] == 0 and kern[".vgpr_spill_count"] == 0, name
        assert kern[".max_flat_workgroup_size"] == (1024 if "scan" in name else 64), name


class _StubEnv:
    """What trajectory_rows reads of an env, without a device."""
    num_envs, n_o, n_u, max_episode_steps, dt = 4, 10, 1, 300, 0.02

    def _trajectory_spec(self):
        import torch
        return {"obs": (10, torch.float32), "u": (1, torch.float32), "reward": (0, torch.float32),
                "done": (0, torch.uint8), "term_obs": (10, torch.float32)}


def _dyn(mode, size=100):
    from rcbf_amd.dynamics import DynamicsModel
    env = types.SimpleNamespace(dynamics_mode=mode, dt=0.02)
    return DynamicsModel(env, types.SimpleNamespace(cuda=False, gp_model_size=size))


@pytest.mark.parametrize("method", ["trajectory_rows", "append_trajectory"])
def test_trajectory_methods_check_their_arguments_before_any_library_call(monkeypatch, method):
    import torch

    from rcbf_amd import _lib

    def no_library():
        raise AssertionError(f"{method} reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    env, dm = _StubEnv(), _dyn("SimulatedCars")
    call = getattr(dm, method)  # host tensors stand in: every check below fails before a launch
    K, B = 3, 4

    def traj(P=64):
        return {"obs": torch.zeros(K, P, 10)[:, :B], "u": torch.zeros(K, P, 1)[:, :B],
                "done": torch.zeros(K, P, dtype=torch.uint8)[:, :B], "term_obs": torch.zeros(K, P, 10)[:, :B]}

    obs0, step0 = torch.zeros(B, 10), torch.zeros(B, dtype=torch.int32)
    for f in ("obs", "u", "done"):
        t = traj()
        del t[f]
        with pytest.raises(ValueError, match=f):
            call(env, t, obs0, step0)
    t = traj()
    del t["term_obs"]  # required with auto_reset ...
    with pytest.raises(ValueError, match="term_obs"):
        call(env, t, obs0, step0)
    with pytest.raises(ValueError, match="HIP device"):  # ... and only then; host tensors are refused last
        call(env, t, obs0, step0, auto_reset=False)
    t = traj()
    t["u"] = torch.zeros(K, 128, 1)[:, :B]  # another pitch
    with pytest.raises(ValueError, match="pitch"):
        call(env, t, obs0, step0)
    t = traj()
    t["done"] = t["done"].to(torch.int32)  # dtype
    with pytest.raises(ValueError, match="done"):
        call(env, t, obs0, step0)
    t = traj()
    t["obs"] = torch.zeros(K, B, 12)[:, :, :10]  # not dense in w
    with pytest.raises(ValueError, match="obs"):
        call(env, t, obs0, step0)
    t = traj()
    t["term_obs"] = torch.zeros(K - 1, 64, 10)[:, :B]  # fewer rows than the others are asked for
    with pytest.raises(ValueError, match="term_obs"):
        call(env, t, obs0, step0, rows=K)
    with pytest.raises(ValueError, match="rows"):
        call(env, traj(), obs0, step0, rows=K + 1)
    with pytest.raises(ValueError, match="rows"):
        call(env, traj(), obs0, step0, rows=0)
    with pytest.raises(ValueError, match="obs0"):
        call(env, traj(), obs0[:, :9], step0)
    with pytest.raises(ValueError, match="obs0"):
        call(env, traj(), obs0.numpy(), step0)
    with pytest.raises(ValueError, match="step0"):
        call(env, traj(), obs0, step0.to(torch.int64))
    with pytest.raises(ValueError, match="every"):
        call(env, traj(), obs0, step0, every=0)
    if method == "trajectory_rows":
        with pytest.raises(ValueError, match="keep_last"):
            call(env, traj(), obs0, step0, keep_last=0)
    else:
        with pytest.raises(ValueError, match="refit"):
            call(env, traj(), obs0, step0, refit="sometimes")
    with pytest.raises(ValueError, match="Unicycle"):  # a cars env's rows into a unicycle model
        getattr(_dyn("Unicycle"), method)(env, traj(), obs0, step0)
    assert dm.history_counter == 0 and not dm.disturbance_history["state"].any()


def test_an_env_batch_of_zero_gives_no_rows_and_no_library_call(monkeypatch):
    import torch

    from rcbf_amd import _lib

    def no_library():
        raise AssertionError("an empty batch reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    env = _StubEnv()
    env.num_envs = 0
    K = 3
    traj = {"obs": torch.zeros(K, 64, 10)[:, :0], "u": torch.zeros(K, 64, 1)[:, :0],
            "done": torch.zeros(K, 64, dtype=torch.uint8)[:, :0], "term_obs": torch.zeros(K, 64, 10)[:, :0]}
    obs0, step0 = torch.zeros(0, 10), torch.zeros(0, dtype=torch.int32)
    for keep_last in (None, 5):
        dm = _dyn("SimulatedCars")
        state, dist, n = dm.trajectory_rows(env, traj, obs0, step0, keep_last=keep_last)
        assert n == 0 and tuple(state.shape) == (0, 10) == tuple(dist.shape) and state.dtype == torch.float64
    for refit in ("every", "last", "none"):
        dm = _dyn("SimulatedCars")
        snaps = _recording(dm)
        assert dm.append_trajectory(env, traj, obs0, step0, refit=refit) == 0
        assert dm.history_counter == 0 and not snaps


def _reference_ring(x, d, cap, counter):
    """dynamics.py:263-290 row by row: ring, counter, (counter, ring copies) at each fit."""
    ring_s, ring_d, fits = np.zeros((cap, x.shape[1])), np.zeros((cap, x.shape[1])), []
    for i in range(x.shape[0]):
        ring_s[counter % cap], ring_d[counter % cap] = x[i], d[i]
        counter += 1
        if counter % (cap / 10) == 0:
            fits.append((counter, ring_s.copy(), ring_d.copy()))
    return ring_s, ring_d, counter, fits


def _recording(dm):
    snaps = []
    dm.fit_gp_model = lambda *a, **k: snaps.append((dm.history_counter, dm.disturbance_history["state"].copy(),
                                                    dm.disturbance_history["disturbance"].copy()))
    return snaps


def test_append_rows_in_ragged_chunks_reproduces_the_row_by_row_ring():
    dm = _dyn("SimulatedCars")
    snaps = _recording(dm)
    rng = np.random.default_rng(12)
    n = 250
    x, d = rng.normal(30, 3, (n, 10)), rng.normal(0, 1, (n, 10))
    ring_s, ring_d, cnt, want = _reference_ring(x, d, 100, 0)
    i = 0
    for k in [1, 37, 5, 10, 3, 60, 19, 100, 15]:
        dm._append_rows(x[i:i + k], d[i:i + k])
        i += k
    assert i == n and dm.history_counter == cnt == n
    assert [c for c, _, _ in snaps] == [c for c, _, _ in want] == list(range(10, 251, 10))
    assert all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(snaps, want))
    assert np.array_equal(dm.disturbance_history["state"], ring_s)
    assert np.array_equal(dm.disturbance_history["disturbance"], ring_d)


@pytest.mark.parametrize("n,counter", [(250, 7), (3, 8), (3, 4), (100, 0), (0, 13), (1037, 95)])
def test_refit_modes_through_a_stubbed_trajectory_rows(n, counter):
    """trajectory_rows stubbed with n known rows (it returns the last keep_last
    of them, as the kernel does): 'every' is the reference's row-by-row state
    and fit points; 'last' and 'none' leave the same ring and counter, 'last'
    fitting once at the end iff a fit point was crossed."""
    import torch
    rng = np.random.default_rng(n + counter)
    x, d = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))
    ring_s, ring_d, cnt, want = _reference_ring(x, d, 100, counter)
    asked = []

    def stub(env, traj, obs0, step0, rows=None, every=2, auto_reset=True, keep_last=None):
        asked.append((rows, every, auto_reset, keep_last))
        m = n if keep_last is None else min(n, keep_last)
        return torch.as_tensor(x[n - m:]), torch.as_tensor(d[n - m:]), n

    for refit in ("every", "last", "none"):
        dm = _dyn("Unicycle")
        dm.history_counter = counter
        dm.trajectory_rows = stub
        snaps = _recording(dm)
        assert dm.append_trajectory(None, None, None, None, rows=5, every=3, auto_reset=False, refit=refit) == n
        assert asked[-1] == (5, 3, False, None if refit == "every" else 100)
        assert dm.history_counter == cnt == counter + n
        assert np.array_equal(dm.disturbance_history["state"], ring_s), refit
        assert np.array_equal(dm.disturbance_history["disturbance"], ring_d), refit
        if refit == "every":
            assert [c for c, _, _ in snaps] == [c for c, _, _ in want]
            assert all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(snaps, want))
        elif refit == "last":
            assert [c for c, _, _ in snaps] == ([cnt] if want else [])
        else:
            assert not snaps


def test_a_ring_size_that_is_no_multiple_of_ten_fits_where_the_reference_does():
    """gp_model_size = 55: a fit every 5.5 rows, i.e. at every 11th."""
    import torch
    n, counter = 40, 3
    rng = np.random.default_rng(1)
    x, d = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))
    ring_s, _, cnt, want = _reference_ring(x, d, 55, counter)
    assert [c for c, _, _ in want] == [11, 22, 33]
    for refit, fits in (("every", [11, 22, 33]), ("last", [43])):
        dm = _dyn("Unicycle", 55)
        dm.history_counter = counter
        dm.trajectory_rows = lambda *a, **k: (torch.as_tensor(x), torch.as_tensor(d), n)
        snaps = _recording(dm)
        dm.append_trajectory(None, None, None, None, refit=refit)
        assert [c for c, _, _ in snaps] == fits and dm.history_counter == cnt
        assert np.array_equal(dm.disturbance_history["state"], ring_s)

"""The edge-avoiding a-trous denoiser (mrt_renderer_denoise; csrc/denoise.hip).  Its definition is tests/denoise_reference.py: on the GPU the kernels
must give that restatement's float32 result bit for bit; on the CPU the restatement itself is shown to do a denoiser's job against the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_STATE = 1, 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rmse(a, b, mask):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)[mask].mean()))


# ---------------------------------------------------------------- D: the filter does its job (CPU)
def test_reference_filter_lowers_the_error_of_a_noisy_cornell_image(mrt, orc):
    """Measured when the defaults were chosen (sigma_color 4, sigma_normal 0.25, sigma_depth 0.25; CornellScene 64 x 64, seed 1, against 512 frames):
    RMSE 1 frame 0.2145 -> 0.1295, 4 frames 0.1313 -> 0.0762."""
    w = h = 64
    sc = mrt.CornellScene((w, h))
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    ref_r = orc.OracleRenderer(osc, w, h, seed=1, max_bounces=3, camera=sc.camera)
    ref_r.render(512, threads=4)
    ref = ref_r.accumulation()
    for frames in (4, 1):
        orr = orc.OracleRenderer(osc, w, h, seed=1, max_bounces=3, camera=sc.camera)
        nd, al, _, _ = D.oracle_guides(orr, sc, frames, osc.intersect_closest)
        noisy = orr.accumulation()
        den = D.denoise_reference(noisy, nd, al, **D.DEFAULTS)
        covered = al[..., 3] > 0
        e_noisy, e_den = _rmse(noisy, ref, covered), _rmse(den, ref, covered)
        print(f"frames {frames}: rmse noisy {e_noisy:.4f} denoised {e_den:.4f}")
        assert e_den < e_noisy, (frames, e_noisy, e_den)
        # the double-precision evaluation of the same expressions stays close to the float32 one
        d64 = D.denoise_reference(noisy, nd, al, dtype=np.float64, **D.DEFAULTS)
        print(f"frames {frames}: max |f32 - f64| = {np.abs(den.astype(np.float64) - d64).max():.3e}")
        assert np.abs(den.astype(np.float64) - d64).max() < 1e-3
        orr.close()
    ref_r.close(); osc.close()


def test_reference_conventions():
    rng = np.random.default_rng(0)
    h, w = 20, 28
    nd = np.zeros((h, w, 4), np.float32); nd[..., 2] = 1.0; nd[..., 3] = 3.0
    al = np.ones((h, w, 4), np.float32); al[..., :3] = 0.5
    # a constant image comes back bit for bit (0.375 / 0.5 and the products with the B-spline weights are exact)
    acc = np.zeros((h, w, 4), np.float32); acc[..., :3] = 0.375; acc[..., 3] = 1.0
    out = D.denoise_reference(acc, nd, al, 5, 4.0, 0.25, 0.25, 1)
    assert np.array_equal(_bits(out), _bits(acc))
    # a pixel whose neighbours all face away by more than sigma_normal keeps its value; so does everything under demodulate = 0 there
    acc = rng.uniform(0.1, 2.0, (h, w, 4)).astype(np.float32); acc[..., 3] = 1.0
    nd2 = nd.copy(); nd2[7, 9, :3] = (1.0, 0.0, 0.0)
    out = D.denoise_reference(acc, nd2, al, 3, 4.0, 0.25, 0.25, 0)
    # (every weight but the centre's is 0, so an iteration computes (9/64 * x) / (9/64): two roundings of relative error <= 2^-24 each — the value is kept
    # to 2^-23 per iteration, not always to the bit: 9 is not a power of two)
    assert np.abs(out[7, 9].astype(np.float64) - acc[7, 9]).max() <= 3 * 2.0 ** -23 * acc[7, 9].max()
    assert np.abs(out[7, 10].astype(np.float64) - acc[7, 10]).max() > 1e-3            # its neighbour, which has like-minded neighbours, is filtered
    # a pixel without coverage passes through and is nobody's tap
    al2 = al.copy(); al2[5, 5] = 0.0
    acc2 = acc.copy(); acc2[5, 5, :3] = 1000.0
    o1 = D.denoise_reference(acc, nd, al2, 3, 4.0, 0.25, 0.25, 0); o2 = D.denoise_reference(acc2, nd, al2, 3, 4.0, 0.25, 0.25, 0)
    assert np.array_equal(_bits(o2[5, 5, :3]), _bits(acc2[5, 5, :3]))
    m = np.ones((h, w), bool); m[5, 5] = False
    assert np.array_equal(_bits(o1[m]), _bits(o2[m]))
    # ... to the bit under demodulation too, whatever its value (its A is 1, not max(0, 1e-3))
    al3 = al.copy(); al3[:, :3] = 0.0
    acc3 = rng.uniform(0.01, 9.0, (h, w, 4)).astype(np.float32); acc3[..., 3] = 1.0
    o3 = D.denoise_reference(acc3, nd, al3, 5, 4.0, 0.25, 0.25, 1)
    assert np.array_equal(_bits(o3[:, :3, :3]), _bits(acc3[:, :3, :3])) and not np.array_equal(o3[:, 3:, :3], acc3[:, 3:, :3])


# ---------------------------------------------------------------- C: the kernels equal the definition (GPU)
def _sky(mrt, size):
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="plane", position=[0, 0, 0], scale=10)]
    return S(size)


def _check(r, **params):
    acc, g = r.accumulation(), r.guides()
    out = r.denoise(**params)
    p = dict(D.DEFAULTS); p.update(params)
    ref = D.denoise_reference(acc, g["normal_depth"], g["albedo"], **p)
    diff = _bits(out) != _bits(ref)
    print(f"{params}: {int(diff.any(-1).sum())} of {diff.shape[0] * diff.shape[1]} pixels differ, max |d| = {np.abs(out.astype(np.float64) - ref).max():.3e}")
    assert not diff.any(), f"{params}: {int(diff.any(-1).sum())} pixels differ from the float32 restatement"
    assert np.array_equal(_bits(r.accumulation()), _bits(acc)), "the accumulation buffer was modified"
    return out, acc, g


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [1, 4])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_denoise_equals_reference_cornell(mrt, gpu_ctx, orc, frames, iterations):
    r = mrt.Renderer((64, 64), mrt.CornellScene((64, 64)), ctx=gpu_ctx, seed=1)
    try:
        r.set_option("guides", 1)
        r.draw(frames, wait=True)
        out, _, _ = _check(r, iterations=iterations)
        assert np.array_equal(r.denoised_tonemapped(), orc.tonemap_rgba8(out))
        assert np.array_equal(_bits(r.denoised()), _bits(out))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("params", [{}, {"demodulate": 0}, {"sigma_color": 0.7, "sigma_normal": 0.1, "sigma_depth": 0.05, "iterations": 4}, {"iterations": 8}])
def test_denoise_equals_reference_ragged(mrt, gpu_ctx, params):
    r = mrt.Renderer((37, 23), mrt.CornellScene((37, 23)), ctx=gpu_ctx, seed=4)
    try:
        r.set_option("guides", 1)
        r.draw(3, wait=True)
        _check(r, **params)
    finally:
        r.close()


@pytest.mark.gpu
def test_denoise_dragon_scene_with_many_edges(mrt, gpu_ctx):
    sc = mrt.DragonScene((96, 54)); sc.models = [m for m in sc.models if m.name != "dragon"]
    r = mrt.Renderer((96, 54), sc, ctx=gpu_ctx, seed=2)
    try:
        r.set_option("guides", 1)
        r.draw(4, wait=True)
        _check(r)
    finally:
        r.close()


@pytest.mark.gpu
def test_sky_pixels_pass_through_and_are_never_taps(mrt, gpu_ctx):
    import torch
    w, h = 64, 48
    r = mrt.Renderer((w, h), _sky(mrt, (w, h)), ctx=gpu_ctx, seed=1)
    try:
        r.set_option("guides", 1)
        r.draw(4, wait=True)
        out, acc, g = _check(r)
        never = g["albedo"][..., 3] == 0
        assert never.any() and (~never).any()
        assert np.array_equal(_bits(out[never][:, :3]), _bits(acc[never][:, :3]))
        # another colour in the never-hit pixels changes no covered pixel
        # (arbitrary floats there: copied through means to the bit for any value — A = 1 where nothing was hit, not accum / 1e-3 * 1e-3)
        acc2 = acc.copy(); acc2[never, :3] = np.random.default_rng(3).uniform(0.01, 9.0, (int(never.sum()), 3)).astype(np.float32)
        t = torch.from_numpy(acc2).to("cuda:0")
        r.write_accum_from(t.data_ptr(), acc2.nbytes); r.wait(); torch.cuda.synchronize()
        out2, _, _ = _check(r)
        assert np.array_equal(_bits(out2[~never]), _bits(out[~never]))
        assert np.array_equal(_bits(out2[never][:, :3]), _bits(acc2[never][:, :3]))
        assert not np.array_equal(out2[never], out[never])
        # the denoised image into a tensor
        d = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        r.copy_denoised_to(d.data_ptr(), d.numel() * 4); r.wait(); torch.cuda.synchronize()
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(out2))
    finally:
        r.close()


@pytest.mark.gpu
def test_denoise_errors(mrt, gpu_ctx):
    r = mrt.Renderer((32, 32), mrt.CornellScene((32, 32)), ctx=gpu_ctx)
    try:
        def code(fn, *a, **k):
            with pytest.raises(mrt.MRTError) as e: fn(*a, **k)
            return e.value.code
        assert code(r.denoise) == ERR_STATE                          # guides off
        r.set_option("guides", 1)
        assert code(r.denoise) == ERR_STATE                          # no frame yet
        r.draw(1, wait=True)
        assert code(r.denoised) == ERR_STATE and code(r.denoised_tonemapped) == ERR_STATE          # no denoise yet
        for bad in ({"iterations": 0}, {"iterations": 9}, {"sigma_color": 0.0}, {"sigma_normal": -1.0}, {"sigma_depth": float("nan")}, {"sigma_color": float("inf")}, {"demodulate": 2}):
            assert code(r.denoise, **bad) == ERR_INVALID, bad
        r.denoise()
        buf = np.zeros((32, 32, 4), np.float32)
        assert mrt.lib.mrt_renderer_read_denoised(r.handle, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 4) == ERR_INVALID
        assert mrt.lib.mrt_renderer_denoise(r.handle, None) == 0          # NULL = the defaults
        assert np.array_equal(_bits(r.denoised()), _bits(r.denoise()))
        r.set_shard(0, 2)
        r.draw(1, wait=True)
        assert code(r.denoise) == ERR_STATE                          # sharded: the neighbours are elsewhere
    finally:
        r.close()


# ---------------------------------------------------------------- E: the C++ mirror
@pytest.mark.gpu
def test_cpp_mirror_guides_and_denoise_match_python(mrt, gpu_ctx, tmp_path):
    exe, out = str(tmp_path / "denoise_host"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "denoise_host.cpp"),
                           "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-o", exe])
    w, h, frames = 96, 54, 3
    p = subprocess.run([exe, str(w), str(h), str(frames), out], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    raw = open(out, "rb").read()
    n = w * h * 16
    assert len(raw) == 4 * n + w * h * 4
    r = mrt.Renderer((w, h), mrt.DragonScene((w, h)), ctx=gpu_ctx)
    try:
        r.set_option("guides", 1)
        r.draw(frames, wait=True)
        g = r.guides(); den = r.denoise(); img = r.denoised_tonemapped()
        assert raw[0:n] == g["normal_depth"].tobytes() and raw[n:2 * n] == g["albedo"].tobytes() and raw[2 * n:3 * n] == g["ids"].tobytes()
        assert raw[3 * n:4 * n] == den.tobytes() and raw[4 * n:] == img.tobytes()
    finally:
        r.close()


def test_cpp_mirror_denoise_host_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "denoise_host.cpp")])

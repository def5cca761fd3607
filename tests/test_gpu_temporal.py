"""GPU tests of the seed offset (sptr_set_seed_offset) and of the denoiser's temporal reprojection
(sptr_set_denoise_history): DESIGN.md §6f.

Configurations as tests/test_gpu_denoise.py: 150x82 (ragged 32x8 blocks and 32x32 tiles on both edges) of the
scene default (BVH2 staged in LDS) and of the 30x70 sphere mesh with set_bvh_width(4) (the wide walk from L2).

The reprojection and the per-pixel-sigma filter are compared bit for bit with the numpy restatement
(tests/temporal_ref.py) fed the GPU's own accumulation, AOV planes and carried history: tests/test_gpu_denoise.py
finds k_aov's depth bit-equal to intersect on the numpy pixel-centre directions, so those directions are the
device's and zero differing pixels is required.

A lane context refuses the history calls as it refuses sptr_set_denoise; the ABI hands no lane context out,
so that refusal has no test here."""
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import oracle
import sptr
import temporal_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 150, 82
ITER = 3
CONFIGS = [("default", 0, 0, 0), ("sphere_mesh", 30, 70, 4)]
TARGET = (0.0, 1.0, 0.0)
# cameras a few pixels apart: the default one and two more on its orbit about the target (3 and 6 degrees)
POSITIONS = [(0.0, 3.0, 8.0), (0.41869, 3.0, 7.98904), (0.83623, 3.0, 7.95618)]


def _reset(r):
    r.set_seed_offset(0)
    r.set_denoise_history(0)
    r.set_denoise(0)
    r.set_pixel_lanes(0)
    r.set_launch_mode(0)
    r.set_bvh_width(0)


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def cfg(request, renderer):
    name, p0, p1, width = request.param
    _reset(renderer)
    renderer.set_bvh_width(width)
    sptr.setup_default(renderer, name, p0, p1)
    cams = [sptr.camera_lookat(pos=p, target=TARGET, aspect=W / H) for p in POSITIONS]
    # the wave buffers at their largest size of this module, so that no later call grows them (a growth is
    # a state change: it drops the history as it drops the AOV cache)
    renderer.render(cams[0], W, H, spp=4)
    yield {"name": name, "p": (p0, p1), "cams": cams, "lds": width == 0}
    _reset(renderer)


def _read_aovs(r):
    nz = np.concatenate([r.read_aov(sptr.SPTR_AOV_NORMAL), r.read_aov(sptr.SPTR_AOV_DEPTH)[..., None]], axis=-1)
    return nz, r.read_aov(sptr.SPTR_AOV_ALBEDO), r.read_aov(sptr.SPTR_AOV_ID)


def _state(r, history=True):
    """What the last call left: accumulation, AOV planes, filtered image, RGB8 and (history on) the history image
    and its info."""
    nz, albedo, ids = _read_aovs(r)
    s = {"acc": r.read_accum(), "nz": nz, "albedo": albedo, "ids": ids, "den": r.read_denoised(), "rgb": r.read_rgb8()}
    if history:
        s["hist"] = r.read_history()
        s["info"] = r.history_info()
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _differing(a, b):
    """Finite pixels of b that differ from a in any bit (the non-finite ones must be non-finite in both)."""
    fin = np.isfinite(b).all(axis=-1)
    assert np.array_equal(fin, np.isfinite(a).all(axis=-1))
    return int((_bits(a)[fin] != _bits(b)[fin]).any(axis=-1).sum()), int(fin.sum())


# ---------------------------------------------------------------------------------------- 1. the seed offset
def test_seed_offset_renders_the_oracles_frame(cfg, renderer):
    k = 5
    cam = cfg["cams"][0]
    renderer.set_denoise(0)
    renderer.set_seed_offset(k)
    renderer.render(cam, W, H, spp=1)
    acc, rgb = renderer.read_accum(), renderer.read_rgb8()
    renderer.set_seed_offset(0)
    P = oracle.Prepared(oracle.builtin_scene(cfg["name"], *cfg["p"]), bvh=True)
    oacc, _, _ = P.render(cam.as_array(), W, H, oracle.preset_materials(False), oracle.default_lights(), frames=1,
                          frame_begin=k + 1, threads=8)
    orgb = oracle.resolve(oacc, 1)  # (the oracle's own image divides by its frame_begin: the divisor here is 1)
    same = float((rgb == orgb).all(axis=2).mean())
    m = np.isfinite(acc) & np.isfinite(oacc)
    rel = float(np.abs(acc[m] - oacc[m]).sum() / np.abs(oacc[m]).sum())
    print(f"{cfg['name']}: offset {k} against the oracle's frame {k + 1}: identical RGB8 {same:.5f}, relative L1 {rel:.2e}")
    assert (~m).sum() <= 3 and same >= 0.999 and rel <= 1e-3


def test_seed_offset_zero_and_continuation(cfg, renderer):
    cam = cfg["cams"][0]
    renderer.set_denoise(0)
    renderer.render(cam, W, H, spp=3)
    plain = renderer.read_accum()
    renderer.set_seed_offset(0)
    renderer.render(cam, W, H, spp=3)
    assert np.array_equal(_bits(renderer.read_accum()), _bits(plain))  # offset 0: the accumulation as before
    # the offset moves the seeds only: reset, continuity and divisor follow frame_begin
    renderer.set_seed_offset(5)
    renderer.render(cam, W, H, spp=2)
    one, rgb = renderer.read_accum(), renderer.read_rgb8()
    renderer.render(cam, W, H, spp=1, frame_begin=1)
    renderer.render(cam, W, H, spp=1, frame_begin=2)
    assert np.array_equal(_bits(renderer.read_accum()), _bits(one)) and np.array_equal(renderer.read_rgb8(), rgb)
    assert not np.array_equal(one, plain)
    # frames 6 and 7 of the plain accumulation: what frames 1..7 hold beyond frames 1..5, up to the sums' rounding
    renderer.set_seed_offset(0)
    renderer.render(cam, W, H, spp=5)
    five = renderer.read_accum().astype(np.float64)
    renderer.render(cam, W, H, spp=2, frame_begin=6)
    seven = renderer.read_accum().astype(np.float64)
    m = np.isfinite(seven).all(axis=-1) & np.isfinite(one).all(axis=-1)
    rel = float(np.abs((seven - five)[m] - one[m]).sum() / np.abs(one[m]).sum())
    print(f"{cfg['name']}: offset 5 x 2 frames against frames 6..7 of one accumulation: relative L1 {rel:.2e}")
    assert rel <= 1e-5  # float32 sums of 7 terms: 2^-24 x a few, relative to two of the terms


def test_seed_offset_in_two_lanes_and_graph_replays(cfg, renderer):
    cam = cfg["cams"][0]
    renderer.set_denoise(0)
    renderer.set_seed_offset(5)
    out = []
    for lanes, mode in ((1, 1), (2, 1), (1, 3), (2, 3)):
        renderer.set_pixel_lanes(lanes)
        renderer.set_launch_mode(mode)
        for _ in range(3):  # (the shape repeats: mode 3 replays the graph it captured)
            renderer.render(cam, W, H, spp=2)
        assert renderer.pixel_lanes_info()["active"] == (lanes == 2 and cfg["lds"])
        out.append(renderer.read_accum())
    renderer.set_pixel_lanes(0)
    renderer.set_launch_mode(0)
    renderer.set_seed_offset(0)
    for a in out[1:]:
        assert np.array_equal(_bits(a), _bits(out[0]))
    renderer.render(cam, W, H, spp=2)
    assert not np.array_equal(renderer.read_accum(), out[0])  # (the offset was honoured in each of them)


# ---------------------------------------------------------------------------------------- 2. no carry
@pytest.mark.parametrize("n", [1, 3])
def test_no_carry_equals_the_filter_without_history(cfg, renderer, n):
    renderer.set_denoise(ITER)
    renderer.set_denoise_history(8)
    renderer.render(cfg["cams"][0], W, H, spp=n)
    s = _state(renderer)
    renderer.set_denoise_history(0)
    ref = D.denoise(s["acc"], n, s["nz"], s["albedo"], ITER)
    bad, fin = _differing(s["den"], ref)
    print(f"{cfg['name']} n={n}: {bad} of {fin} finite pixels differ from denoise_ref.denoise")
    assert bad == 0
    assert s["info"]["reprojected"] == 0 and not s["info"]["carried"]
    hit = s["nz"][..., 3] >= 0
    assert np.array_equal(_bits(s["hist"][..., 0:3]), _bits(D.mean(s["acc"], n)))
    assert (s["hist"][hit, 3] == n).all() and (s["hist"][~hit, 3] == 0).all()
    renderer.render(cfg["cams"][0], W, H, spp=n)  # history off again: the same bytes
    assert np.array_equal(renderer.read_rgb8(), s["rgb"]) and np.array_equal(_bits(renderer.read_denoised()), _bits(s["den"]))


# ---------------------------------------------------------------------------------------- 3. the restatement
def test_moves_are_bit_equal_to_the_restatement(cfg, renderer):
    M = 2  # (the cap bites at the third camera)
    renderer.set_denoise(ITER)
    renderer.set_denoise_history(M)
    carry, took = None, []
    for cam, n in zip(cfg["cams"], (2, 1, 1)):
        renderer.render(cam, W, H, spp=n)
        s = _state(renderer)
        den, hist, cnt = T.denoise(s["acc"], n, s["nz"], s["albedo"], s["ids"], cam.as_array(), carry, M, ITER)
        bad_h, fin = _differing(s["hist"], hist)
        bad_d, _ = _differing(s["den"], den)
        hit = s["nz"][..., 3] >= 0
        print(f"{cfg['name']} n={n}: history {bad_h}, filtered {bad_d} of {fin} finite pixels differ from the restatement; "
              f"{s['info']['reprojected']} of {int(hit.sum())} hits took history, {s['info']['ms_reproject']:.4f} ms")
        assert bad_h == 0 and bad_d == 0
        assert s["info"]["reprojected"] == cnt and s["info"]["carried"] == (carry is not None)
        assert np.array_equal(s["hist"][..., 3] > n, (hist[..., 3] > n))
        took.append(cnt)
        carry = {"hist": s["hist"], "nz": s["nz"], "ids": s["ids"], "cam": cam.as_array()}
    renderer.set_denoise_history(0)
    hits = int((s["nz"][..., 3] >= 0).sum())
    assert took[0] == 0 and took[1] > hits // 2 and took[2] > hits // 2  # (the test saw history taken)
    assert s["hist"][..., 3].max() == 1 + M  # (and the cap reached)


# ---------------------------------------------------------------------------------------- 4. a standing camera
def test_standing_camera_converges_to_the_accumulation(cfg, renderer):
    cam = cfg["cams"][0]
    renderer.set_denoise(ITER)
    renderer.set_denoise_history(8)
    for k in range(4):
        renderer.set_seed_offset(k)
        renderer.render(cam, W, H, spp=1)
    hist, nz = renderer.read_history(), _read_aovs(renderer)[0]
    renderer.set_seed_offset(0)
    renderer.set_denoise_history(0)
    renderer.render(cam, W, H, spp=4)
    mean4 = D.mean(renderer.read_accum(), 4)
    ok = (nz[..., 3] >= 0) & np.isfinite(mean4).all(axis=-1)
    assert ok.sum() > 1000
    rel = float(np.abs(hist[ok, 0:3].astype(np.float64) - mean4[ok]).sum() / np.abs(mean4[ok].astype(np.float64)).sum())
    print(f"{cfg['name']}: m' in [{hist[ok, 3].min():.6f}, {hist[ok, 3].max():.6f}], t_0 against the 4-frame mean: "
          f"relative L1 {rel:.2e}")
    assert np.abs(hist[ok, 3] - 4.0).max() <= 1e-3
    assert rel <= 1e-3


# ---------------------------------------------------------------------------------------- 5. the carry rules
def test_the_carry_is_dropped_by_state_size_and_setter(cfg, renderer):
    a, b = cfg["cams"][0], cfg["cams"][1]
    renderer.set_denoise(ITER)
    renderer.render(b, W, H, spp=1)
    plain = renderer.read_denoised()  # the filter without history
    renderer.set_denoise_history(8)
    renderer.render(a, W, H, spp=1)
    renderer.render(b, W, H, spp=1)
    assert renderer.history_info()["carried"] and renderer.history_info()["reprojected"] > 0
    assert not np.array_equal(renderer.read_denoised(), plain)  # (a carry does change the result)

    def drops(between):
        renderer.render(a, W, H, spp=1)
        between()
        renderer.render(b, W, H, spp=1)
        info = renderer.history_info()
        assert not info["carried"] and info["reprojected"] == 0
        assert np.array_equal(_bits(renderer.read_denoised()), _bits(plain))

    drops(lambda: renderer.set_materials(sptr.preset_materials(with_light=False)))
    drops(lambda: renderer.render(a, 64, 48, spp=1))
    drops(lambda: renderer.set_denoise_history(8))
    renderer.set_denoise_history(0)


def test_four_single_frames_equal_one_call_of_four_with_the_same_carry(cfg, renderer):
    a, b = cfg["cams"][0], cfg["cams"][1]
    renderer.set_denoise(ITER)
    out = []
    for calls in ((1, 1, 1, 1), (4,)):
        renderer.set_denoise_history(8)  # (drops the history held)
        renderer.render(a, W, H, spp=2)
        done = 0
        for n in calls:
            renderer.render(b, W, H, spp=n, frame_begin=done + 1)
            done += n
            info = renderer.history_info()
            assert info["carried"] and info["reprojected"] > 0
        out.append((renderer.read_history(), renderer.read_denoised(), renderer.read_rgb8()))
    renderer.set_denoise_history(0)
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and np.array_equal(out[0][2], out[1][2])
    hit = out[0][0][..., 3] > 0
    assert out[0][0][hit, 3].max() == 6.0  # n = 4 and the m = 2 of the carry: its own passes were not fed back


# ---------------------------------------------------------------------------------------- 6. invariance
def test_results_do_not_depend_on_how_the_call_is_launched(cfg, renderer):
    a, b = cfg["cams"][0], cfg["cams"][1]
    renderer.set_denoise(0)
    renderer.render(b, W, H, spp=1)
    acc_plain = renderer.read_accum()
    renderer.set_denoise(ITER)

    def sequence(flags=0):
        renderer.set_denoise_history(8)
        renderer.render(a, W, H, spp=1, flags=flags)
        renderer.render(b, W, H, spp=1, flags=flags)
        if flags:
            renderer.collect_stats()
        return renderer.read_history(), renderer.read_denoised(), renderer.read_rgb8(), renderer.history_info()["reprojected"]

    base = sequence()
    assert np.array_equal(_bits(renderer.read_accum()), _bits(acc_plain))  # the accumulation is only read
    others = []
    renderer.set_launch_mode(1)
    others.append(sequence())
    renderer.set_launch_mode(0)
    renderer.set_pixel_lanes(2)
    others.append(sequence())
    assert renderer.pixel_lanes_info()["active"] == cfg["lds"]
    renderer.set_pixel_lanes(0)
    others.append(sequence(sptr.SPTR_FRAME_ASYNC))
    renderer.set_denoise_history(0)
    assert base[3] > 0
    for o in others:
        assert np.array_equal(_bits(o[0]), _bits(base[0])) and np.array_equal(_bits(o[1]), _bits(base[1]))
        assert np.array_equal(o[2], base[2]) and o[3] == base[3]


# ---------------------------------------------------------------------------------------- 7. errors
def test_errors():
    """On a context of its own, so that "before any pass" holds."""
    r = sptr.Renderer(0)
    try:
        sptr.setup_default(r, "default")
        cam = sptr.camera_lookat(aspect=W / H)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.set_denoise_history(1025)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.set_denoise_history(4, reserved=(0, 1, 0))
        r.set_denoise_history(1024)
        r.set_denoise(ITER)
        r.width, r.height = W, H
        with pytest.raises(sptr.SptrError):
            r.read_history()  # no pass yet
        assert r.history_info() == {"reprojected": 0, "ms_reproject": 0.0, "carried": False}
        r.render(cam, W, H, spp=1)
        assert r.read_history().shape == (H, W, 4)
        r.set_denoise(0)  # history only acts while the denoiser is on
        r.render(cam, W, H, spp=1)
        with pytest.raises(sptr.SptrError):
            r.read_history()
        r.set_seed_offset(0xFFFFFFFF)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.render(cam, W, H, spp=1)  # 2^32 - 1 + 1 + 1 - 1
        r.set_seed_offset(0xFFFFFFFE)
        r.render(cam, W, H, spp=1)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.render(cam, W, H, spp=1, frame_begin=2)
        r.set_seed_offset(1)
        with pytest.raises(sptr.SptrError, match="rc=-1"):
            r.render(cam, W, H, spp=1, integrator=sptr.SPTR_INTEGRATOR_PATHTRACER)
        r.set_seed_offset(0)
        r.render(cam, W, H, spp=1, integrator=sptr.SPTR_INTEGRATOR_PATHTRACER)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------- the upper layers
def test_cli_history_and_orbit(tmp_path):
    """sptr_cli --history [M] --orbit DEG: HipBackend::Settings::history on a camera that moves every frame."""
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"

    def run(name, *extra):
        out = tmp_path / name
        res = subprocess.run([exe, "--scene", "default", "--w", str(W), "--h", str(H), "--spp", "6", "--denoise", str(ITER),
                              "--orbit", "3", "--json", "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        with open(out, "rb") as f:
            return json.loads(res.stdout.strip().splitlines()[-1]), f.read()

    off, img_off = run("off.ppm")
    on, img_on = run("on.ppm", "--history")
    two, _ = run("two.ppm", "--history", "2")
    assert off["history"] == 0 and off["reprojected"] == 0 and off["ms_reproject"] == 0
    assert on["history"] == sptr.DEFAULT_MAX_HISTORY and two["history"] == 2
    hits = 1000  # (the view holds some 1300 hit pixels; five of the six frames have a carry)
    assert on["reprojected"] > hits * 5 / 6 and two["reprojected"] > hits * 5 / 6
    assert on["ms_reproject"] > 0 and on["aov_passes"] == 6
    assert img_on != img_off

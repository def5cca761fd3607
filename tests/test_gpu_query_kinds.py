"""GPU tests of what the four query kinds share on the host (csrc/sptr_api.cpp: the run records, query_scratch, the
enqueue head and tail, the staging table of host-pointer calls; sptr.py: _query_arrays and Renderer._query_call):
sptr_query_rays, sptr_query_multi_hit, sptr_query_points and sptr_query_signed_distance next to each other.

Scenes: tests/refit_common.py's two, default_emitter (staged into LDS) and the 30x70 sphere mesh with set_bvh_width(4)
(the BVH walked from L2), uploaded after set_signed_distance().  Rays are refit_common's, points points_common's
(repeated to the size a step needs).  There is no reference model here: the assertion is byte equality with the
same query issued alone, and of one way to ask with another; what the answers are is the other query tests' matter."""
import functools

import numpy as np
import pytest
import torch  # before the library, as tests/conftest.py's renderer fixture does: one HIP runtime for both

import points_common as P
import refit_common as R
import sptr

pytestmark = pytest.mark.gpu
K = 3
CALLS = {
    "rays": lambda r, x, **kw: r.query_rays(x, **kw),
    "any_hit": lambda r, x, **kw: r.query_rays(x, any_hit=True, **kw),
    "multi_hit": lambda r, x, **kw: r.query_multi_hit(x, K, **kw),
    "points": lambda r, x, **kw: r.query_points(x, **kw),
    "signed": lambda r, x, **kw: r.query_signed_distance(x, **kw),
}
FIELDS = {"rays": ("geom", "prim", "t", "ng", "uv"), "any_hit": (), "multi_hit": ("geom", "prim", "t", "ng", "uv"),
          "points": P.FIELDS, "signed": P.FIELDS + ("signed_dist", "normal", "feature")}
INFO = {"rays": "query_info", "multi_hit": "multi_hit_info", "points": "point_query_info", "signed": "signed_info"}
# each step outgrows the sort scratch of the one before: the reallocation that has to wait for every kind's last query
GROWING = (("rays", 64), ("points", 4096), ("multi_hit", 8192), ("signed", 16384))


def _context(cfg):
    name, p0, p1, width = cfg
    r = sptr.Renderer(0)
    r.set_bvh_width(width)
    r.set_signed_distance(True)
    r.upload_scene(sptr.builtin_scene(name, p0, p1))
    r.set_materials(sptr.preset_materials(with_light=(name == "default_emitter")))
    r.set_lights(sptr.default_lights())
    r.set_environment(None)
    assert (r.scene_layout()["lds_bytes"] != 0) == (width == 0) and r.signed_info()["valid"] == 1
    return r


@functools.lru_cache(maxsize=None)
def _input(name, kind, n):
    """(n, 8) rays or (n, 4) points of scene `name`, read-only."""
    if kind in ("points", "signed"):
        x = np.resize(P.points(name)[0], (n, 4))
    else:
        x = np.ascontiguousarray(R.rays(sptr.camera_lookat(aspect=R.W / R.H).as_array())[-n:])  # (the random rays)
    assert x.shape == (n, 8 if kind in ("rays", "any_hit", "multi_hit") else 4)
    x.setflags(write=False)
    return x


def _dev(a):
    t = torch.from_numpy(a.copy()).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _same_bytes(got, want, what):
    assert list(got) == list(want), what
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


@functools.lru_cache(maxsize=None)
def _alone(cfg, kind, n):
    """The sorted query of kind and size n, issued alone and synchronously on a fresh context."""
    r = _context(cfg)
    res = _np(CALLS[kind](r, _dev(_input(cfg[0], kind, n)), sort=True))
    r.close()
    for a in res.values():
        a.setflags(write=False)
    return res


@pytest.fixture(scope="module", params=R.SCENES, ids=R.SCENE_IDS)
def scene(request, renderer):
    r = _context(request.param)
    yield request.param, r
    r.close()


@pytest.mark.parametrize("steps", [GROWING, GROWING[::-1]], ids=["growing", "shrinking"])
@pytest.mark.parametrize("cfg", R.SCENES, ids=R.SCENE_IDS)
def test_kinds_back_to_back_on_one_stream(renderer, cfg, steps):
    """Four sorted queries of four kinds enqueued on one stream with nothing between them; growing sizes regrow the
    shared scratch under the queries before, shrinking ones reuse it.  Each equals the query issued alone."""
    want = {kind: _alone(cfg, kind, n) for kind, n in steps}
    r = _context(cfg)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    inputs = {kind: _dev(_input(cfg[0], kind, n)) for kind, n in steps}
    got = {kind: CALLS[kind](r, inputs[kind], sort=True, stream=stream.cuda_stream) for kind, _ in steps}
    stream.synchronize()
    for kind, n in steps:
        _same_bytes(_np(got[kind]), want[kind], f"{cfg[0]} {kind} n={n} on the stream vs alone")
    info = {kind: getattr(r, INFO[kind])() for kind, _ in steps}
    print(cfg[0], info)
    for kind in ("rays", "multi_hit", "points"):
        # (the signed query runs a point query, so the points kind has run two)
        assert info[kind]["queries"] == (2 if kind == "points" else 1) and info[kind]["sorted"] == 1, (kind, info[kind])
        assert info[kind]["ms_sort"] > 0.0
    assert info["signed"]["ms_sign"] > 0.0
    r.close()


@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("kind", list(CALLS))
def test_staging_of_host_pointer_calls(scene, kind, n):
    """The numpy path with every field, then with each field alone: a column does not depend on what else is staged
    (signed_dist alone: the ids are staged though nobody takes them), and the whole equals the device-tensor path."""
    cfg, r = scene
    x = _input(cfg[0], kind, n)
    every = CALLS[kind](r, x)
    assert all(isinstance(a, np.ndarray) for a in every.values())
    head = [k for k in every if k not in FIELDS[kind]]  # multi-hit's count, any-hit's occluded: in every result
    assert list(every) == head + list(FIELDS[kind]) and len(head) == (kind in ("multi_hit", "any_hit"))
    for f in FIELDS[kind]:
        one = CALLS[kind](r, x, fields=(f,))
        _same_bytes(one, {k: every[k] for k in head + [f]}, f"{cfg[0]} {kind} n={n}: {f} alone vs with every field")
    _same_bytes(_np(CALLS[kind](r, _dev(x))), every, f"{cfg[0]} {kind} n={n}: device tensors vs numpy")
    if kind == "any_hit":  # (one field: asked for twice, it is the same)
        _same_bytes(CALLS[kind](r, x), every, f"{cfg[0]} any_hit n={n} again")

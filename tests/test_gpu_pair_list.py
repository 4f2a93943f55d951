"""The masked search's pending-pair list (csrc/pt_kernels.hip: pt_pair_list_build) on the device.

A search whose rays bring candidate masks walks the low mask word lane by lane while many lanes hold a survivor, and lists what is
left of it and the whole high word ONCE, as (triangle, ray lane) pairs the tail's rounds test 64 at a time.  The list is built by
helper lanes: two lanes share the survivors of one ray, whoever owns it.  Here:

  1. renders against the CPU oracle, bit for bit and ray for ray, of scenes of 32, 33, 34, 36 and 64 triangles -- the high word
     empty, one, two, four and all 32 of its bits in use -- at 64 x 64 and at 33 x 97 (partial waves), 4 frames, depth 16; one at
     depth 64; one with PT_OPT_CHUNK_FRAMES = 2, whose checkpoints fall between searches;
  2. the builder alone on masks the renderer rarely reaches (pt_pair_check_kernel): the pairs its rounds would test are, as a
     multiset, the masks' set bits -- every pair exactly once -- and every round but the last tests 64 of them.
"""
import numpy as np
import pytest

import scenes
from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import scene as _scene, shim
from scenes import box_prefix, joined

pytestmark = pytest.mark.gpu

FRAMES = 4


SCENES = {
    32: lambda: box_prefix(32),
    33: lambda: box_prefix(33),
    34: lambda: box_prefix(34),
    36: _scene.load_model,
    64: lambda: joined(_scene.load_model(), scenes.random_quads(105), scenes.random_quads(1007)),
}
SIZES = [(64, 64), (33, 97)]


@pytest.fixture(scope="module")
def wanted(oracle):
    """the oracle's renders, each computed once"""
    cache = {}

    def get(ntri, W, H, depth):
        key = (ntri, W, H, depth)
        if key not in cache:
            tris, mats = SCENES[ntri]()
            assert len(tris) == ntri
            with np.errstate(all="ignore"):
                cache[key] = (tris, mats) + tuple(oracle.render(tris, mats, W, H, FRAMES, max_bounces=depth, want_stats=True))
        return cache[key]
    return get


def _compare(device, wanted, ntri, W, H, depth):
    tris, mats, want, st = wanted(ntri, W, H, depth)
    got, gst = render(device, tris, mats, W, H, FRAMES, depth=depth, want_stats=True)
    what = "%d triangles, %d x %d, depth %d" % (ntri, W, H, depth)
    assert_fb_equal(got, want, what)
    assert gst[shim.PT_STAT_RAYS] == st["rays"], "%s: %d rays, the oracle traced %d" % (what, gst[shim.PT_STAT_RAYS], st["rays"])
    assert gst[shim.PT_STAT_SAMPLES] == st["samples"] == W * H * FRAMES


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("ntri", sorted(SCENES))
def test_render_matches_the_oracle(device, wanted, ntri, W, H):
    _compare(device, wanted, ntri, W, H, 16)


def test_render_matches_the_oracle_at_depth_64(device, wanted):
    _compare(device, wanted, 36, 64, 64, 64)


def test_render_matches_the_oracle_with_checkpoints_between_searches(device, wanted):
    with options(device, CHUNK_FRAMES=2):
        _compare(device, wanted, 36, 33, 97, 16)


# ---- the builder alone ---------------------------------------------------------------------------------------------------------
CAP = 4096   # pairs of a case: 64 lanes x 64 triangles at the most


def _run(device, masks, ntri):
    """masks: (cases, 64, 2) uint32 -> per case (pairs tested, rounds, the pairs in the order tested)"""
    from oclpathtracer_amd import adl

    masks = np.ascontiguousarray(masks, np.uint32)
    cases = masks.shape[0]
    assert masks.shape == (cases, 64, 2)
    k = device.getKernel("PtShimTest", "PairCheckKernel")
    assert k is not None
    mbuf = adl.Buffer(device, cases * 128, np.uint32)
    obuf = adl.Buffer(device, cases * (2 + CAP), np.uint32)
    try:
        mbuf.write(masks.reshape(-1), cases * 128)
        obuf.write(np.full(cases * (2 + CAP), 0xFFFFFFFF, np.uint32), cases * (2 + CAP))
        launcher = adl.Launcher(device, k)
        launcher.setBuffers([adl.BufferInfo(mbuf), adl.BufferInfo(obuf)])
        launcher.setConst(np.int32(ntri))
        launcher.setConst(np.uint32(cases))
        launcher.setConst(np.uint32(CAP))
        launcher.launch1D(1)
        res = np.empty(cases * (2 + CAP), np.uint32)
        obuf.read(res, cases * (2 + CAP))
        device.waitForCompletion()
    finally:
        mbuf.release()
        obuf.release()
    res = res.reshape(cases, 2 + CAP)
    return [(int(r[0]), int(r[1]), r[2:2 + min(int(r[0]), CAP)]) for r in res]


def _expected(case, ntri):
    """the set bits of a case's masks as pairs (triangle << 6 | lane): low word bit nlo-1-j <-> triangle j, high word bit
    ntri-33-j <-> triangle 32+j (a high word counts where the scene has more than 32 triangles)"""
    nlo, nhi = min(ntri, 32), max(ntri - 32, 0)
    out = []
    for lane in range(64):
        lo, hi = int(case[lane, 0]), int(case[lane, 1])
        out += [((nlo - 1 - b) << 6) | lane for b in range(32) if lo >> b & 1]
        if nhi:
            out += [((32 + nhi - 1 - b) << 6) | lane for b in range(32) if hi >> b & 1]
    return np.sort(np.array(out, np.uint32))


def _valid(masks, ntri):
    """only bits of triangles the scene has (what the mask tables hold); at 32 triangles or fewer the high word is left as it is:
    the search must not read it"""
    m = np.array(masks, np.uint32)
    nlo, nhi = min(ntri, 32), max(ntri - 32, 0)
    m[..., 0] &= np.uint32((1 << nlo) - 1)
    if nhi:
        m[..., 1] &= np.uint32((1 << nhi) - 1)
    return m


def _with_total(rng, total):
    """exactly `total` set bits, anywhere in the 64 x 64"""
    bits = np.zeros(64 * 64, bool)
    bits[rng.choice(64 * 64, total, replace=False)] = True
    return np.packbits(bits.reshape(64, 2, 32), axis=-1, bitorder="little").view(np.uint32).reshape(64, 2)


def _random(rng, n):
    """n draws: a density of set bits and a share of live lanes each, from almost nothing to almost everything"""
    out = []
    for _ in range(n):
        p = rng.choice([0.01, 0.03, 0.1, 0.3, 0.7])
        live = rng.random(64) < rng.choice([0.05, 0.3, 0.5, 1.0])
        bits = (rng.random((64, 2, 32)) < p) & live[:, None, None]
        if rng.random() < 0.3:
            bits[:, 1, :] = False
        out.append(np.packbits(bits, axis=-1, bitorder="little").view(np.uint32).reshape(64, 2))
    return out


def _cases():
    rng = np.random.default_rng(20261021)
    ones = np.uint32(0xFFFFFFFF)
    named = {}
    named["all lanes empty"] = np.zeros((64, 2), np.uint32)
    one = np.zeros((64, 2), np.uint32)
    one[37] = ones
    named["one lane with 64 bits"] = one
    named["every lane all ones"] = np.full((64, 2), ones, np.uint32)
    for total in (63, 64, 65, 128, 129):
        named["a total of %d" % total] = _with_total(rng, total)
    high = np.zeros((64, 2), np.uint32)
    high[:, 1] = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    named["bits only in the high word"] = high
    dead = rng.integers(0, 1 << 32, (64, 2), dtype=np.uint64).astype(np.uint32)
    dead[1::2] = 0
    named["dead lanes interleaved"] = dead
    dead2 = rng.integers(0, 1 << 32, (64, 2), dtype=np.uint64).astype(np.uint32) & np.uint32(0x00410208)
    dead2[0::3] = 0
    named["dead lanes interleaved, few bits"] = dead2
    names = list(named) + ["random draw %d" % i for i in range(200)]
    return names, np.stack(list(named.values()) + _random(rng, 200))


def _check(device, names, masks, ntri):
    got = _run(device, masks, ntri)
    rounds_seen = 0
    for name, case, (count, rounds, pairs) in zip(names, masks, got):
        what = "%s, %d triangles" % (name, ntri)
        want = _expected(case, ntri)
        assert count == len(want), "%s: %d pairs tested, the masks hold %d" % (what, count, len(want))
        assert np.array_equal(np.sort(pairs), want), "%s: the pairs tested are not the masks' set bits, each once" % what
        assert rounds == (len(want) + 63) // 64, "%s: %d rounds for %d pairs" % (what, rounds, len(want))
        rounds_seen += rounds
    return rounds_seen


def test_every_pair_is_listed_exactly_once_at_64_triangles(device):
    names, masks = _cases()
    assert len(names) == 211 and int(np.unpackbits(masks[2].view(np.uint8)).sum()) == 4096
    rounds = _check(device, names, masks, 64)
    print("%d cases, %d rounds" % (len(names), rounds))


@pytest.mark.parametrize("ntri", [1, 20, 32, 33, 36, 63])
def test_every_pair_is_listed_exactly_once_at_other_counts(device, ntri):
    """the words' offsets: a low word of fewer than 32 triangles, a high word of 1, 4 and 31 -- and at 32 or fewer a high word that
    must not count, whatever it holds"""
    names, masks = _cases()
    _check(device, names[:61], _valid(masks[:61], ntri), ntri)

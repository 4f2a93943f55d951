"""tests/masked_search_cases.py on the CPU: the expectation the GPU test compares with is the oracle's, and the inputs reach what
they were made for.  Every condition here is one on the reference and the inputs alone: where one fails the inputs change, not the
threshold.  The measured figures are printed beside the conditions."""
import os
import subprocess

import numpy as np
import pytest

import masked_search_cases as msc
import query_oracle
import scenes
from test_secondary_masks_cpu import records

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", msc.NAMES)
def test_the_model_is_the_oracle(name):
    """with the full mask the model is query_oracle.closest on the whole scene in index, t, u, v; its accepted pairs are all_hits"""
    tris, rays = msc.scene(name)
    tab = msc.table(name)
    n = len(rays)
    got = tab.winner(np.arange(n), np.ones((n, len(tris)), bool))
    h = query_oracle.closest(tris, rays)
    want = np.stack([h[:, 1].view(np.uint32), h[:, 0].view(np.uint32), h[:, 2].view(np.uint32), h[:, 3].view(np.uint32)], axis=1)
    miss = h[:, 1].view(np.int32) < 0
    want[miss, 1] = msc.MISS_T            # (the query's miss has t = +inf, the search's the tmax it started from)
    assert np.array_equal(got, want), "%s: %d rays differ" % (name, int((got != want).any(axis=1).sum()))
    ray, tri, t = query_oracle.all_hits(tris, rays)
    j, r = np.nonzero(tab.acc)
    order = np.lexsort((j, r))
    assert np.array_equal(r[order], ray) and np.array_equal(j[order], tri), name + ": the accepted pairs are not all_hits'"
    assert np.array_equal(tab.t[j[order], r[order]], t.view(np.uint32)), name + ": other t than all_hits'"
    assert (~miss).sum() > 0 or len(tris) == 1
    print("%s: %d rays, %d accepted pairs, %d hits" % (name, n, len(ray), int((~miss).sum())))


def test_the_sheets_reach_the_dense_regime():
    tris, rays = msc.scene("sheets")
    tab = msc.table("sheets")
    n = len(rays)
    count = tab.acc.sum(axis=0)
    print("accepted triangles per ray: mean %.2f (>= 6), share with 24 or more %.3f (>= 0.10), most %d" % (count.mean(), (count >= 24).mean(), count.max()))
    assert count.mean() >= 6
    assert (count >= 24).mean() >= 0.10
    win = tab.winner(np.arange(n), np.ones((n, 64), bool))[:, 0].astype(np.int64)
    hit = win != 0xFFFFFFFF
    lowest = tab.acc.argmax(axis=0)
    not_lowest = (hit & (win != lowest)).mean()
    low, high = (hit & (win < 32)).mean(), (hit & (win >= 32)).mean()
    print("winner not the lowest accepted index: %.3f of the rays (>= 0.30); winners in the low word %.3f, in the high word %.3f (>= 0.10 each)" % (not_lowest, low, high))
    assert not_lowest >= 0.30
    assert low >= 0.10 and high >= 0.10
    tied, first, second = msc.ties(tab)
    print("rays whose two nearest accepted hits tie in t: %d (>= 30)" % len(tied))
    assert len(tied) >= 30
    assert (first < second).all() and np.array_equal(win[tied], first), "a tie is not won by the lower index"
    for src, dst in scenes.SHEET_COPIES:
        decided = int(np.isin(first, (2 * src, 2 * src + 1)).sum())
        mine = np.isin(first, (2 * src, 2 * src + 1))
        assert np.array_equal(second[mine], first[mine] + 2 * (dst - src)), "quad %d ties with another than its copy %d" % (src, dst)
        print("quad %d and its copy %d decide %d ties (>= 5)" % (src, dst, decided))
        assert decided >= 5
    assert (first // 32 != second // 32).any() and (first // 32 == second // 32).any(), "ties within a word and across the words"
    # the few non-finite rays are there and accept nothing
    bad = ~np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all(axis=1)
    assert bad.sum() == 8 and count[bad].sum() == 0


@pytest.mark.parametrize("name", msc.NAMES)
def test_the_cases_are_what_they_say(name):
    tab = msc.table(name)
    cs = msc.cases(name)
    ntri = tab.ntri
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    for k in msc.LIVE_LOW:
        for c in cs:
            if "%d lanes with low-word survivors" % k in c.name:
                assert c.low_owners() == k, c.name
    for c in cs:
        assert c.mask.shape == (64, 2) and c.want.shape == (64, 4)
        assert not (c.mask[:, 0] >> np.uint32(min(ntri, 32) - 1) >> np.uint32(1)).any(), c.name + ": low-word bits above the scene's triangles"
        if ntri > 32:
            assert not (c.mask[:, 1] >> np.uint32(ntri - 33) >> np.uint32(1)).any(), c.name + ": high-word bits above the scene's triangles"
        assert (c.want[~c.alive] == [0xFFFFFFFF, msc.MISS_T, 0, 0]).all(), c.name + ": a dead lane expects a hit"
        if "every valid bit" in c.name or "a superset" in c.name:
            whole = tab.winner(c.ray, np.ones((64, ntri), bool))
            assert np.array_equal(c.want, whole), c.name + ": a superset of the accepted set must give the unmasked closest hit"
        if "a garbage high word" in c.name:
            assert c.mask[:, 1].all()
        if "every second lane dead" in c.name:
            assert c.alive.sum() == 32 and c.mask[~c.alive].any(axis=1).all()
        if "one lane with every bit" in c.name:
            assert sorted(c.bits.sum(axis=1))[-2:] == [0, ntri]
    hits = sum(int((c.want[:, 0] != 0xFFFFFFFF).sum()) for c in cs)
    rounds = [(c.pairs() + 63) // 64 for c in cs]
    print("%s: %d waves, %d lanes expect a hit, up to %d pairs in a wave, %d waves with more than two rounds' worth" % (
        name, len(cs), hits, max(c.pairs() for c in cs), sum(r > 2 for r in rounds)))
    assert hits > 0 or ntri == 1
    if name in ("sheets", "sheets_33", "sheets_63"):
        # (the scenes that hold a quad and its copy) lanes whose mask keeps both triangles of a tie for the nearest hit
        tied, first, second = msc.ties(tab)
        a, b = np.full(tab.acc.shape[1], -1), np.full(tab.acc.shape[1], -1)
        a[tied], b[tied] = first, second
        asked = sum(int((c.alive & (a[c.ray] >= 0) & c.bits[np.arange(64), a[c.ray]] & c.bits[np.arange(64), b[c.ray]]).sum()) for c in cs)
        print("%s: %d lanes are asked to break a tie" % (name, asked))
        assert asked >= 64
    if name == "sheets":
        # the runner-up family asks something: where the accepted set holds two, another triangle wins
        wo = [c for c in cs if "without its winner" in c.name]
        assert sum(int((c.want[:, 0] != 0xFFFFFFFF).sum()) for c in wo) >= 64
        assert sum(r > 2 for r in rounds) >= 20, "few waves wrap the 128-entry ring"
        assert len(cs) >= 60


def test_the_cases_are_a_few_hundred_waves():
    total = sum(len(msc.cases(n)) for n in msc.NAMES)
    print("%d waves in all" % total)
    assert 200 <= total <= 400


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("masked_search") / "secondary_masks_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe,
                           os.path.join(HERE, "secondary_masks_check.cpp")])
    return exe


# (alternate, the least mean number of accepted triangles per primary ray the renders of tests/test_gpu_masked_search.py count on)
@pytest.mark.parametrize("alternate,least", [(False, 12.0), (True, 5.0)])
def test_the_sheet_renders_reach_the_dense_regime(checker, tmp_path, alternate, least):
    """the host's secondary-mask table stands for the scene, and the oracle accepts many triangles per primary ray of the 64 x 64 render's
    four frames (about 1 on the Cornell box)"""
    tris, _ = scenes.sheets(alternate=alternate)
    rec = str(tmp_path / "records.f32")
    records(tris).tofile(rec)
    out = subprocess.check_output([checker, "valid", rec, str(len(tris))]).decode()
    print(out.strip())
    assert out.startswith("invalid 0 of 64"), out
    mean = msc.primary_accepted(tris, 64, 64, 4)
    print("accepted triangles per primary ray: %.2f (>= %.0f)" % (mean, least))
    assert mean >= least

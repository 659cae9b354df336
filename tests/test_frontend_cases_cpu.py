"""The cases of tests/test_gpu_frontend_geometry.py without a GPU (tests/frontend_cases.py builds them for both files): every
condition that makes them worth running, from the oracle and the restated admission rules alone.

  * the restated rules are the source's, read from its text; admit() gives the facts the geometry table states;
  * taken together the geometries run every byte shift of the horizontal pass at widths that are no multiple of 4, every tap
    count of both passes up to the LDS plan's limit, one and ten trips of the load loop, and all four combinations of passes;
  * every limit is admitted and its neighbour refused for the named reason;
  * the oracle's resampler equals Pillow's at every geometry (test_frontend_oracle.py pins it at eight others);
  * a frame whose single extreme were lost would give another plane (the "steps_*" kinds; the two-level kinds cannot show it);
  * the host C implementation equals the oracle on every frame, the sizes only the device refuses included.
"""
import re

import numpy as np
import pytest

import frame_frontend as ff
import frontend_cases as fc


def _facts(H, W, C=3):
    f = fc.admit(H, W, C)
    assert isinstance(f, fc.Facts), ((H, W, C), f)
    return f


def test_the_restated_rules_are_the_sources():
    fe, eng = fc.source("ga3c_frontend.hpp"), fc.source("ga3c_engine.hip")
    assert (fc.FE_THREADS, fc.FE_MAXG, fc.FE_MAXK, fc.IMG, fc.LDS_LIMIT) == (1024, 10, 8, 84, 150 * 1024)
    assert fc.MAX_PIXELS == 40960
    # the four rules in the order admit() takes them, and the texts REFUSED is matched against
    rules = [r"if \(npx % 4 \|\| npx > \(int64_t\)4 \* FE_MAXG \* FE_THREADS\)", r"if \(th\.ksize > FE_MAXK\) return fail",
             r"f\.lds = frontend_lds_bytes\(height, width, IMG, IMG, f\.hks, f\.vks\);", r"if \(f\.lds > 150 \* 1024\) return fail"]
    at = [re.search(r, eng).start() for r in rules]
    assert at == sorted(at)
    assert re.search(r"make_bilinear_table\(width, IMG\), tv = make_bilinear_table\(height, IMG\)", eng)
    for text in ("3 or 4 channels", "one channel means ready-made %dx%d planes", "height*width must be a multiple of 4 and at most %d",
                 "width %d needs %d taps per output, the kernel holds %d", "a %dx%d frame does not fit the kernel's LDS plan"):
        assert text in eng, text
    # frontend_lds_bytes and the kernel's own LDS map
    assert re.search(r"tab = \(\(size_t\)\(OH \* \(2 \+ vks\) \+ OW \* \(2 \+ hks\)\) \* 4 \+ 15\) & ~\(size_t\)15;", fe)
    assert re.search(r"g8 = \(\(size_t\)H \* W \+ 15\) & ~\(size_t\)15;\s+return tab \+ g8 \+ \(\(\(size_t\)H \* OW \+ 15\) & ~\(size_t\)15\);", fe)
    # the code the derived facts describe
    assert re.search(r"const int idx = y \* a\.W \+ xmin\[q\];", fe) and re.search(r"const uint32_t sh = \(uint32_t\)\(idx & 3\) \* 8;", fe)
    assert re.search(r"if \(a\.hks > 5\) \{", fe) and re.search(r"if \(a\.W != a\.OW\) \{", fe) and re.search(r"if \(a\.H != a\.OH\) \{", fe)
    assert re.search(r"for \(int j = 0; j < FE_MAXG; \+\+j\) \{\s+const int grp = tid \+ j \* FE_THREADS;", fe)
    assert re.search(r"for \(int k = 0; k < n; \+\+k\) \{", fe)
    # the plane history's two rules
    assert (fc.HIST_ARGS_MAX_B, fc.GATHER_MAX_BLOCKS) == (192, 512)
    assert re.search(r"if \(batch <= %d\) \{\s+for \(int i = 0; i < batch; \+\+i\) \{ hr\.seq\[i\]" % fc.HIST_ARGS_MAX_B, eng)
    assert re.search(r"i \+= \(int64_t\)gridDim\.x \* blockDim\.x\)", fe)
    # ksize is odd, so "at most FE_MAXK = 8" means at most 7: a width of 3 x 84
    assert all(ff.bilinear_coeffs(w, fc.IMG)[0] % 2 == 1 for w in range(1, 400))
    assert ff.bilinear_coeffs(252, fc.IMG)[0] == 7 and ff.bilinear_coeffs(253, fc.IMG)[0] == 9


def test_admit_gives_the_facts_of_the_geometry_table():
    f = _facts(210, 160)
    assert (f.hks, f.vks, f.trips) == (5, 7, 9)
    assert _facts(4, 1).n_h == {1} and _facts(4, 1).trips == 1 and _facts(2, 2).trips == 1
    for g in ((12, 7), (20, 3)):
        assert g[1] % 2 == 1 and _facts(*g).trips == 1 and _facts(*g).hks == 3
    f = _facts(84, 83)
    assert f.hks == 3 and f.n_h == {1, 2} and f.pass3 and not f.pass4
    f = _facts(84, 85)
    assert f.hks == 5 and f.n_h == {2} and not f.pass4
    assert _facts(52, 168).hks == 5
    f = _facts(52, 169)
    assert f.hks == 7 and f.n_h == {3, 4, 5}
    f = _facts(160, 252)
    assert f.hks == 7 and f.n_h == {4, 5, 6} and f.trips == 10
    assert 250 % 4 == 2 and _facts(162, 250).hks == 7 and _facts(100, 101).idx3 == {0, 1, 2, 3}
    assert (_facts(83, 84).vks, _facts(85, 84).vks) == (3, 5) and not _facts(83, 84).pass3 and _facts(83, 84).pass4
    f = _facts(480, 84)
    assert f.vks == 13 and (min(f.n_v), max(f.n_v)) == (9, 12)
    assert _facts(253, 160).vks == 9 and max(_facts(253, 160).n_v) == 6 and max(_facts(256, 160).n_v) == 7
    f = _facts(296, 138)
    assert f.vks == 9 and f.n_v == {5, 7, 8} and f.trips == 10 and f.partial and f.hks == 5        # a tap count past 7 ...
    # ... whose eighth tap has a weight: 300 rows have 8 taps too, the last of them zero
    assert [fc.live_taps(h) for h in (250, 253, 256, 296, 300, 480)] == [6, 6, 7, 8, 7, 12] and _facts(300, 136).n_v == {5, 7, 8}
    f = _facts(256, 160)
    assert 256 * 160 == fc.MAX_PIXELS and f.trips == fc.FE_MAXG and not f.partial
    f = _facts(1568, 4)
    assert f.vks == 39 and f.lds == 153440 and max(f.n_v) == 38
    assert _facts(1569, 4).lds == 153552
    f = _facts(84, 84)
    assert not f.pass3 and not f.pass4
    assert isinstance(fc.admit(84, 84, 1), fc.Facts)
    # four channels change nothing but the bytes loaded
    assert all(fc.admit(h, w, 4) == fc.admit(h, w, 3) for h, w in fc.GEOMETRIES)


def test_the_geometries_together_run_every_path():
    facts = {g: _facts(*g) for g in fc.GEOMETRIES}
    two_pass = [g for g, f in facts.items() if f.pass3 and f.pass4]
    assert {g[1] % 4 for g in two_pass} == {0, 1, 2, 3}
    # at a width that is no multiple of 4 the shift depends on the row: all four values at some such geometry ...
    assert any(g[1] % 4 and f.idx3 == {0, 1, 2, 3} for g, f in facts.items())
    # ... and `xmin & 3` is another shift at some (row, output) of EVERY geometry with W % 4 != 0, and of no other
    for (H, W), f in facts.items():
        if not f.pass3:
            continue
        xmin = ff.bilinear_coeffs(W, fc.IMG)[1][:, 0].astype(np.int64)
        idx = np.arange(H)[:, None] * W + xmin[None, :]
        assert ((idx & 3) != (xmin[None, :] & 3)).any() == (W % 4 != 0), (H, W)
    assert {f.hks for f in facts.values() if f.pass3} == {3, 5, 7}
    assert set().union(*(f.n_h for f in facts.values())) == {1, 2, 3, 4, 5, 6}
    assert {f.vks for f in facts.values() if f.pass4} == {3, 5, 7, 9, 13, 33, 39, 41}
    assert set().union(*(f.n_v for f in facts.values())) >= set(range(1, 13)) - {10, 11} | {23, 31, 28, 38, 39}
    trips = {f.trips for f in facts.values()}
    assert {1, fc.FE_MAXG} <= trips and any(f.trips == fc.FE_MAXG and f.partial for f in facts.values())
    assert any(f.trips == fc.FE_MAXG and not f.partial for f in facts.values())
    assert {(f.pass3, f.pass4) for f in facts.values()} == {(True, True), (True, False), (False, True), (False, False)}
    # both sides of the `hks > 5` branch, and frames that leave 1023 threads with the reduction's identities alone
    assert (facts[(52, 168)].hks, facts[(52, 169)].hks) == (5, 7)
    assert all(g[0] * g[1] == 4 for g in ((4, 1), (2, 2)))
    assert set(fc.QUEUE_GEOMETRIES) <= set(two_pass) and all(g[1] % 4 for g in fc.QUEUE_GEOMETRIES)
    order = fc.order_large_small_large()
    assert sorted(order) == sorted(fc.GEOMETRIES)
    px = [h * w for h, w in order]
    assert all(px[i] >= px[i + 1] if i % 2 == 0 else px[i] <= px[i + 1] for i in range(len(px) - 1))     # 84x85 and 85x84 tie
    assert px[0] == fc.MAX_PIXELS and px[1] == 4 and len({(px[i] > px[i + 1]) for i in range(0, 16, 2)}) == 1


def test_every_limit_is_admitted_and_its_neighbour_refused():
    for H, W, C, rule in fc.REFUSED:
        r = fc.admit(H, W, C)
        assert isinstance(r, fc.Refusal) and r.rule == rule, ((H, W, C), r)
    for inside, outside in fc.LIMITS:
        assert inside in fc.GEOMETRIES and outside in [r[:3] for r in fc.REFUSED]
        _facts(*inside)
    # widths: 252 is the widest admitted and 253 the first refused, whatever the height
    assert [w for w in range(1, 400) if isinstance(fc.admit(4, w, 3), fc.Facts)][-1] == 252
    # pixels: 256 rows of 160 fill the ten trips, and one row more is refused for the pixel count, not for LDS
    assert fc.admit(257, 160, 3).rule == "pixels" and fc.lds_bytes(257, 160, 5, 9) < fc.LDS_LIMIT
    assert fc.admit(210, 161, 3).rule == "pixels" and 210 * 161 % 4 == 2 and 210 * 161 < fc.MAX_PIXELS
    # LDS at W = 4: among heights that are a multiple of 4, 1568 is the tallest admitted and 1572 the first refused.  By the
    # rule as the source states it 1569 is admitted too (H*W is a multiple of 4 for every H at W = 4, and rounding g8 and tmp
    # up to 16 leaves it 48 bytes), and 1570 is the first refused.
    ok = [h for h in range(1500, 1600) if isinstance(fc.admit(h, 4, 3), fc.Facts)]
    assert ok == list(range(1500, 1570))
    assert [h for h in ok if h % 4 == 0][-1] == 1568 and fc.admit(1572, 4, 3).rule == "lds" and fc.admit(1570, 4, 3).rule == "lds"
    assert fc.LDS_LIMIT - _facts(1568, 4).lds == 160 and fc.LDS_LIMIT - _facts(1569, 4).lds == 48
    # no admitted frame needs more LDS than those: the search over every height at every width
    def ksize(n):                                                    # ff.bilinear_coeffs(n, 84)[0] without the tables
        return 2 * -(-max(n, fc.IMG) // fc.IMG) + 1
    assert all(ksize(n) == ff.bilinear_coeffs(n, fc.IMG)[0] for n in (1, 83, 84, 85, 168, 169, 252, 253, 1569))
    need = [(fc.lds_bytes(h, w, ksize(w), ksize(h)), h, w) for w in range(1, 253) for h in range(1, fc.MAX_PIXELS // w + 1)
            if (h * w) % 4 == 0]
    fit = [n for n in need if n[0] <= fc.LDS_LIMIT]
    assert sorted(n for n in fit if n[0] == fc.LDS_LIMIT) == [(fc.LDS_LIMIT, 1214, 32), (fc.LDS_LIMIT, 1274, 26)]     # all of it
    assert (153552, 1569, 4) in fit and (153440, 1568, 4) in fit
    assert fc.admit(1276, 26, 3).rule == "lds" and fc.admit(1275, 26, 3).rule == "pixels"
    # the tallest frame of all is one pixel wide, and has the most vertical taps
    assert max((h, w) for _, h, w in fit) == (1616, 1) and max(ksize(h) for _, h, w in fit) == 41 == _facts(1616, 1).vks
    assert fc.admit(1620, 1, 3).rule == "lds" and max(_facts(1616, 1).n_v) == 39


@pytest.mark.parametrize("geom", fc.GEOMETRIES + tuple(r[:2] for r in fc.REFUSED if r[3] in ("taps", "pixels", "lds")))
def test_the_resampler_equals_pillow_at_every_geometry(geom):
    Image = pytest.importorskip("PIL.Image")
    h, w = geom
    rng = np.random.default_rng(h * 1000 + w)
    imgs = [rng.integers(0, 256, size=(h, w), dtype=np.uint8)]
    if geom in fc.QUEUE_GEOMETRIES + tuple(g for g, _ in fc.LIMITS):
        imgs.append((np.add.outer(np.arange(h), np.arange(w)) % 256).astype(np.uint8))
    for img in imgs:
        got = ff.pil_bilinear_u8(img, fc.IMG, fc.IMG)
        whole = np.asarray(Image.fromarray(img, "L").resize((fc.IMG, fc.IMG), resample=Image.BILINEAR))
        # pass by pass, each a resize of its own: Pillow's resampler in ImagingResample's order, whatever Image.resize does
        across = Image.fromarray(img, "L").resize((fc.IMG, h), resample=Image.BILINEAR)
        assert across.size == (fc.IMG, h)
        assert np.array_equal(got, np.asarray(across.resize((fc.IMG, fc.IMG), resample=Image.BILINEAR)))
        if h <= fc.TALL_FOR_PILLOW * w:
            assert np.array_equal(got, whole)
        else:
            # H > 100 W: this Pillow's Image.resize runs the vertical pass first (see frontend_cases.TALL_FOR_PILLOW), an older
            # one does not.  Either way its result is one of the two orders of the same two passes
            down =Image.fromarray(img, "L").resize((w, fc.IMG), resample=Image.BILINEAR)
            first_down = np.asarray(down.resize((fc.IMG, fc.IMG), resample=Image.BILINEAR))
            assert np.array_equal(whole, got) or np.array_equal(whole, first_down)


def test_which_geometries_pillow_resizes_in_the_other_order():
    tall = [g for g in fc.GEOMETRIES if g[0] > fc.TALL_FOR_PILLOW * g[1]]
    assert tall == [(1568, 4), (1569, 4), (1616, 1)]
    assert [r[:2] for r in fc.REFUSED if r[0] > fc.TALL_FOR_PILLOW * r[1]] == [(1572, 4), (1570, 4), (1620, 1)]
    # 1274x26, the frame at the LDS limit itself, is not among them: Image.resize as a whole is held up to 33 vertical taps
    assert 1274 <= fc.TALL_FOR_PILLOW * 26 and fc.admit(1274, 26, 3).vks == 33


def _scaled_without(gray, pixel=None):
    """The 8-bit grey image of ff.preprocess_u8 with the frame's min and max taken over every pixel BUT `pixel`: what a
    reduction that lost the thread, the lane, the wave or the trip holding it would make of the frame."""
    rest = gray.reshape(-1) if pixel is None else np.delete(gray.reshape(-1), pixel)
    cmin, cscale = rest.min(), rest.max() - rest.min()
    scaled = (gray - cmin) * (255.0 / (cscale if cscale != 0 else 1))
    return (scaled.clip(0, 255) + 0.5).astype(np.uint8)


def test_a_lost_extreme_would_show_in_the_plane():
    # the structured kinds are grey (r = g = b): their f64 grey image is a table of 256 entries, looked up
    lut = fc.grey_lut()
    for g, k in (((12, 7), 7), ((100, 101), 9), ((84, 84), 4)):
        assert np.array_equal(lut[fc.case(*g).rgb3[k, :, :, 0]], ff.rgb2gray(fc.case(*g).rgb3[k]))
    for H, W in fc.GEOMETRIES:
        cs = fc.case(H, W)
        npx = H * W
        for kind, level in fc.SINGLE.items():
            k = fc.KINDS.index(kind)
            px = cs.rgb3[k].reshape(npx, 3)
            at = fc.outlier_pixel(kind, npx)
            assert (np.delete(px, at, axis=0) == level).all() and (px[at] == 255 - level).all()
            assert (cs.planes[k] != level).any() and len(np.unique(cs.planes[k])) > 1, (H, W, kind)
            # ... which says the pixel reaches the plane.  Whether its being the EXTREME matters: a lost minimum shows (every
            # pixel then maps to 0), a lost maximum does not (max == min means scale 255 / 1, and 255 x 255 clamps to 255)
            gray = lut[cs.rgb3[k, :, :, 0]]
            whole, without = _scaled_without(gray), _scaled_without(gray, at)
            assert np.array_equal(whole, ff.bytescale(gray))
            assert np.array_equal(whole, without) if level == 0 else not without.any(), (H, W, kind)
        for kind in fc.STEPS:
            k = fc.KINDS.index(kind)
            at = fc.outlier_pixel(kind, npx)
            grey = cs.rgb3[k].reshape(npx, 3)[:, 0].astype(int)
            assert len(np.unique(np.delete(grey, at))) == 2 and grey[at] in (0, 255) and np.sum(grey == grey[at]) == 1
            # the grey image differs at every pixel of the middle level, which goes to an end of the range ...
            gray = lut[cs.rgb3[k, :, :, 0]]
            whole, without = _scaled_without(gray), _scaled_without(gray, at)
            middle = grey == (100 if grey[at] == 255 else 155)
            assert middle.any() and np.array_equal((whole != without).reshape(-1), middle), (H, W, kind)
            assert (np.abs(whole.astype(int) - without)[whole != without] == 155).all()
            # ... and so does the plane (resampled for two of the kinds: the last trip's maximum, the last wave's minimum)
            if kind in ("steps_last", "steps_z15"):
                assert not np.array_equal(ff.pil_bilinear_u8(without, fc.IMG, fc.IMG), cs.planes[k]), (H, W, kind)
        # where the frame has a group for thread 1023, the last wave's last lane holds an extreme in its first trip
        for kind in ("steps_w15", "steps_z15"):
            grp = fc.outlier_pixel(kind, npx) // 4
            assert grp == (fc.FE_THREADS - 1 if npx // 4 >= fc.FE_THREADS else npx // 4 - 1)
        # the last pixel sits in the last (partial) trip; at 256x160 that trip is thread 1023's tenth
        assert (fc.outlier_pixel("steps_last", npx) // 4) // fc.FE_THREADS == fc.admit(H, W, 3).trips - 1
    assert sum(h * w // 4 >= fc.FE_THREADS for h, w in fc.GEOMETRIES) >= 12
    assert (256 * 160 // 4 - 1) % fc.FE_THREADS == fc.FE_THREADS - 1


def test_the_alpha_byte_is_there_and_does_not_matter():
    for H, W in fc.GEOMETRIES:
        cs = fc.case(H, W)
        assert cs.rgb3.shape == (len(fc.KINDS), H, W, 3) and cs.rgb4.shape == (len(fc.KINDS), H, W, 4)
        assert np.array_equal(cs.rgb4[..., :3], cs.rgb3) and cs.planes.shape == (len(fc.KINDS), fc.IMG, fc.IMG)
        if H * W >= 16:
            assert len(np.unique(cs.rgb4[..., 3])) > 4
        for k in (0, 1 + (H + W) % 11):                # a random frame and one of the kinds whose grey image was taken per colour
            assert np.array_equal(ff.preprocess_u8(cs.rgb4[k]), cs.planes[k])
    # the kinds are what they are called
    cs = fc.case(210, 160)
    k = {name: i for i, name in enumerate(fc.KINDS)}
    assert len(np.unique(cs.rgb3[k["uniform"]])) == 256 and set(np.unique(cs.rgb3[k["narrow"]])) == {100, 101, 102, 103}
    assert len(np.unique(cs.rgb3[k["constant"]].reshape(-1, 3), axis=0)) == 1
    assert 2 <= len(np.unique(cs.rgb3[k["rects"]].reshape(-1, 3), axis=0)) <= 7
    assert len(np.unique(cs.planes[k["constant"]])) == 1 and cs.planes[k["constant"]][0, 0] == 0


def test_host_preprocess_equals_the_oracle_at_every_geometry():
    """ga3c_frame_preprocess keeps its scratch and its table cache per thread: large, small, large re-uses both across
    geometries.  The sizes only the device refuses go through it too."""
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.host_lib()
    extra = tuple(r[:2] for r in fc.REFUSED if r[3] in ("taps", "pixels", "lds"))
    assert len(extra) == 7
    for H, W in fc.order_large_small_large(fc.GEOMETRIES + extra):
        cs = fc.case(H, W)
        for C, rgb in ((3, cs.rgb3), (4, cs.rgb4)):
            got = np.full((len(fc.KINDS), fc.IMG, fc.IMG), 7, np.uint8)
            for k in range(len(fc.KINDS)):
                frame = np.ascontiguousarray(rgb[k])
                nat.check_host(lib.ga3c_frame_preprocess(nat.ptr(frame, nat.u8p), H, W, C, fc.IMG, fc.IMG, nat.ptr(got[k], nat.u8p)))
            assert fc.first_difference(got, cs.planes) is None, ((H, W, C), fc.first_difference(got, cs.planes))


def test_the_history_batches_hold_the_rows_they_are_meant_to():
    live = fc.history_live()
    assert len(live) == 208 == fc.HIST_AGENTS * 13 and len(set(live)) == 208 and max(fc.HIST_SIZES) == 208
    assert {s for _, s in live} == set(range(6, 19))
    # the grid's second trip starts with row 74's last groups: 74 rows fit 510 workgroups, 75 do not fit 512
    assert [fc.gather_trips(b) for b in (1, 74, 75, 192, 193, 208)] == [(1, 7), (1, 510), (2, 512), (3, 512), (3, 512), (3, 512)]
    assert 74 * 1764 == 130536 <= 510 * 256 and 75 * 1764 == 132300 > 512 * 256
    assert (fc.HIST_ARGS_MAX_B in fc.HIST_SIZES) and (fc.HIST_ARGS_MAX_B + 1 in fc.HIST_SIZES) and fc.HIST_TRAIN_SIZE == 193
    for B in fc.HIST_SIZES:
        names = fc.history_batch(B)
        assert len(names) == B and set(names) <= set(live)
        if B < 75:
            assert len(set(names)) == B
            continue
        # rows of the grid's second trip: from row 74's 537th group on.  At 75 rows that is the last row alone (row 0's name
        # again); from 192 rows on all four made rows lie there
        first_second_trip = (fc.GATHER_MAX_BLOCKS * 256) // (fc.IMG * fc.IMG // 4)
        assert first_second_trip == 74 and B - 1 >= first_second_trip and (B == 75 or B - 4 >= first_second_trip)
        tail = names[B - 4:]
        assert fc.wraps(tail[0][1]) and tail[0][1] != fc.HIST_PUSHES - 1
        assert fc.HIST_PUSHES - (tail[1][1] - 3) == fc.HIST_DEPTH                     # the oldest admissible plane
        assert tail[2][1] == fc.HIST_PUSHES - 1 and fc.wraps(tail[2][1])              # the newest
        assert tail[3] == names[0] and len(set(names)) < B                            # the same name twice
        assert len(set(names)) >= B - 4
    # states of different names differ, and a state is its four planes, oldest first
    s = fc.history_state(3, 16)
    p = fc.history_planes()
    assert s.shape == (84, 84, 4) and s.dtype == np.uint8 and np.array_equal(s[:, :, 0], p[13, 3, :, :, 0]) and np.array_equal(s[:, :, 3], p[16, 3, :, :, 0])
    q = ff.FrameQueue()
    for t in range(17):
        q.push(p[t, 3, :, :, 0])
    assert np.array_equal(q.state_u8(), s)

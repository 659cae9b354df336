"""The cases of tests/test_frontend_cases_cpu.py and tests/test_gpu_frontend_geometry.py (not collected: no test_ prefix): the
device frame front-end (ga3c_amd/csrc/ga3c_frontend.hpp) at the frame geometries ga3c_net_frames_config admits, and the plane
history past one pass of gather_history_kernel's grid.  Both files build their cases here, so the conditions the CPU file
asserts are the conditions of the frames the GPU file runs.

    admit(H, W, C)        ga3c_net_frames_config's rules and frontend_lds_bytes restated -> Refusal(rule, text) or Facts
    GEOMETRIES, REFUSED   frame sizes on both sides of every rule and at every path of the kernel (tests/README.md has the table)
    KINDS, frames(..)     the content of a geometry's frames; case(H, W) -> both channel counts and the oracle's planes, cached
    history_batch(B)      (agent, plane) names of a batch of B training rows out of 16 agents x 19 pushes, history 16

The constants are read from the source text, not restated: a changed FE_MAXG moves the limits these cases sit on, and the CPU
file's assertions about them then fail instead of testing the old limits.  No case or condition here touches a kernel."""
import collections
import functools
import os
import re

import numpy as np

import frame_frontend as ff

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ga3c_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


_FE, _ENG, _KER = source("ga3c_frontend.hpp"), source("ga3c_engine.hip"), source("ga3c_kernels.hpp")
FE_THREADS = _int(r"constexpr int FE_THREADS = (\d+);", _FE)
FE_MAXG = _int(r"constexpr int FE_MAXG = (\d+);", _FE)
FE_MAXK = _int(r"constexpr int FE_MAXK = (\d+);", _FE)
IMG = _int(r"constexpr int IMG = (\d+),", _KER)
_lds = re.search(r"if \(f\.lds > (\d+) \* (\d+)\) return fail", _ENG)
LDS_LIMIT = int(_lds.group(1)) * int(_lds.group(2))
MAX_PIXELS = 4 * FE_MAXG * FE_THREADS
HIST_ARGS_MAX_B = _int(r"struct HistRows \{ int64_t seq\[(\d+)\];", _FE)       # rows whose names ride in the launch argument
GATHER_MAX_BLOCKS = _int(r"if \(blocks > (\d+)\) blocks = \1;", _ENG)          # gather_history_kernel's grid cap, 256 threads each


def _r16(n):
    return (n + 15) & ~15


def lds_bytes(H, W, hks, vks):
    """frontend_lds_bytes(H, W, IMG, IMG, hks, vks): [resample tables][g8: H*W][tmp: H*IMG], each rounded up to 16."""
    return _r16((IMG * (2 + vks) + IMG * (2 + hks)) * 4) + _r16(H * W) + _r16(H * IMG)


Refusal = collections.namedtuple("Refusal", "rule text")
Facts = collections.namedtuple("Facts", "hks vks n_h n_v idx3 trips partial lds pass3 pass4")
# hks, vks     taps per output the tables hold (ksize of ff.bilinear_coeffs), horizontal and vertical
# n_h, n_v     the set of tap COUNTS of the outputs (bounds[:, 1]); empty for a pass that does not run
# idx3         the set of (y*W + xmin) & 3 over all rows and outputs: the byte shifts pass 3 applies (empty when it does not run)
# trips        trips of the pass-1 / pass-2 loop the busiest thread takes, partial: the last of them leaves threads idle
# pass3        the horizontal pass runs (W != 84); pass4: the vertical pass resamples (H != 84), else it unpacks


def admit(H, W, C):
    """ga3c_net_frames_config(max_agents >= 1, H, W, C) in the order of its checks."""
    if H < 1 or W < 1 or C not in (1, 3, 4):
        return Refusal("channels", "3 or 4 channels")
    if C == 1:
        if (H, W) != (IMG, IMG):
            return Refusal("planes", "one channel means ready-made %dx%d planes" % (IMG, IMG))
        return Facts(0, 0, frozenset(), frozenset(), frozenset(), 0, False, 0, False, False)       # plane_push_kernel: no arithmetic
    hks, hb, _ = ff.bilinear_coeffs(W, IMG)
    vks, vb, _ = ff.bilinear_coeffs(H, IMG)
    npx = H * W
    if npx % 4 or npx > MAX_PIXELS:
        return Refusal("pixels", "height\\*width must be a multiple of 4 and at most %d" % MAX_PIXELS)
    if hks > FE_MAXK:
        return Refusal("taps", "width %d needs %d taps per output, the kernel holds %d" % (W, hks, FE_MAXK))
    lds = lds_bytes(H, W, hks, vks)
    if lds > LDS_LIMIT:
        return Refusal("lds", "a %dx%d frame does not fit the kernel's LDS plan" % (H, W))
    pass3, pass4 = W != IMG, H != IMG
    idx3 = frozenset(((np.arange(H)[:, None] * W + hb[:, 0][None, :]) & 3).ravel().tolist()) if pass3 else frozenset()
    ngrp = npx // 4
    return Facts(hks, vks, frozenset(hb[:, 1].tolist()) if pass3 else frozenset(), frozenset(vb[:, 1].tolist()) if pass4 else frozenset(),
                 idx3, -(-ngrp // FE_THREADS), ngrp % FE_THREADS != 0, lds, pass3, pass4)


def live_taps(n_in):
    """The most taps of an output of the n_in -> 84 table up to and including its last non-zero weight: the tap count of
    Pillow's bounds includes a last tap whose triangle weight is exactly zero at some sizes (300 rows: 8 taps, 7 live)."""
    _, b, k = ff.bilinear_coeffs(n_in, IMG)
    return max(max(i + 1 for i in range(b[o, 1]) if k[o, i] != 0) for o in range(IMG))


# (H, W).  The last three came out of the CPU file's search over every admitted size: 1569x4 is the tallest frame at W = 4 by
# the rule as the source states it (rounding g8 and tmp up to 16 leaves it 48 bytes; 1568 is the tallest H that is a multiple
# of 4), 1274x26 is one of the two admitted frames whose LDS plan is the limit itself, 153,600 bytes, and 1616x1 is the
# tallest frame of all, with the most vertical taps (41).  296x138 came out of a trial (tests/README.md): 253x160 and 256x160 have
# tables 9 taps wide of which no output uses more than 7; at 296 rows some use 8, none of them with weight zero (live_taps).
GEOMETRIES = ((210, 160), (4, 1), (2, 2), (12, 7), (20, 3), (84, 83), (84, 85), (100, 101), (52, 168), (52, 169), (160, 252),
              (162, 250), (83, 84), (85, 84), (480, 84), (253, 160), (256, 160), (1568, 4), (84, 84), (1569, 4), (1274, 26),
              (1616, 1), (296, 138))
# (H, W, C, rule)
REFUSED = ((4, 253, 3, "taps"), (210, 161, 3, "pixels"), (257, 160, 3, "pixels"), (1572, 4, 3, "lds"), (1570, 4, 4, "lds"),
           (1276, 26, 3, "lds"), (1620, 1, 3, "lds"), (210, 160, 2, "channels"), (80, 84, 1, "planes"))
# each limit and the neighbour that the rule refuses
LIMITS = (((160, 252), (4, 253, 3)), ((256, 160), (257, 160, 3)), ((1568, 4), (1572, 4, 3)), ((1569, 4), (1570, 4, 4)),
          ((1274, 26), (1276, 26, 3)), ((1616, 1), (1620, 1, 3)), ((210, 160), (210, 161, 3)))
# Pillow's Image.resize hands a frame with H > 100 W to its resampler in two calls, the vertical pass FIRST (the release
# installed here, 12.2; the releases SciPy <= 1.2 ran on make one call, horizontal pass first, as Resample.c's ImagingResample
# does on its own).  oracle/frame_frontend.py restates ImagingResample, and the host and device front-ends follow it.
TALL_FOR_PILLOW = 100
QUEUE_GEOMETRIES = ((100, 101), (162, 250))


def order_large_small_large(geoms=GEOMETRIES):
    """The geometries by pixel count, taken alternately from the large and the small end: every change of geometry is a change
    of every table and buffer size, in both directions."""
    by_size = sorted(geoms, key=lambda g: g[0] * g[1], reverse=True)
    out = []
    while by_size:
        out.append(by_size.pop(0))
        if by_size:
            out.append(by_size.pop())
    return out


# ---------------------------------------------------------------- content
# Random frames hold 0 and 255 hundreds of times, so they cannot see a min / max reduction that drops a wave, a lane or the
# last partial trip.  The three single-pixel kinds put the frame's min or max in one thread of one wave -- but a kernel that
# LOST a single maximum would still give their planes: with two grey levels in the frame the outlier maps to 255 whatever the
# maximum is taken to be (max == min means scale 255 / 1, and the clamp does the rest).  An extreme is sure to show only
# against a third level: the "steps_*" kinds hold a field of two levels 100 apart and the one outlier, so that a lost extreme
# moves the middle level from 100 (or 155) to 255 (or 0).  "steps_w15" and "steps_z15" put the outlier in the last wave's
# last lane where the frame has a group for it (thread 1023, first trip), else in the last group.
KINDS = ("uniform", "narrow", "constant", "rects", "last255", "first255", "onezero",
         "steps_last", "steps_first", "steps_zero", "steps_w15", "steps_z15")
SINGLE = {"last255": 0, "first255": 0, "onezero": 255}      # kind -> the level of the constant frame it must differ from
STEPS = ("steps_last", "steps_first", "steps_zero", "steps_w15", "steps_z15")


def _two_levels(rng, npx, lo, hi, outlier):
    """npx pixels drawn from {lo, hi}, both present beside the pixel the outlier will take."""
    px = np.where(rng.integers(0, 2, size=npx) == 1, hi, lo).astype(np.uint8)
    a, b = [i for i in range(min(npx, 3)) if i != outlier][:2]
    px[a], px[b] = lo, hi
    return px


def outlier_pixel(kind, npx):
    """The pixel index that holds the frame's single extreme."""
    ngrp = npx // 4
    if kind in ("last255", "steps_last"):
        return npx - 1
    if kind in ("first255", "steps_first"):
        return 0
    if kind in ("onezero", "steps_zero"):
        return npx - 3                                          # in the last group, not its last pixel
    if kind in ("steps_w15", "steps_z15"):
        grp = FE_THREADS - 1 if ngrp >= FE_THREADS else ngrp - 1
        return 4 * grp + 3
    raise KeyError(kind)


def frames(rng, H, W, C):
    """One frame of each of KINDS -> uint8 [len(KINDS), H, W, C].  Grey frames (r = g = b) for the structured kinds, so the
    grey level of a pixel is the byte written; with C = 4 the alpha byte is random."""
    npx = H * W
    out = np.empty((len(KINDS), H, W, C), np.uint8)
    for i, kind in enumerate(KINDS):
        if kind == "uniform":
            f = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        elif kind == "narrow":
            f = (100 + rng.integers(0, 4, size=(H, W, 3))).astype(np.uint8)
        elif kind == "constant":
            f = np.broadcast_to(rng.integers(0, 256, size=3, dtype=np.uint8), (H, W, 3))
        elif kind == "rects":                                  # test_gpu_frontend.atari_like's kind 1, for any frame size
            f = np.empty((H, W, 3), np.uint8)
            f[:] = rng.integers(0, 256, size=(1, 1, 3), dtype=np.uint8)
            for _ in range(6):
                y, x = rng.integers(0, max(1, H - 16)), rng.integers(0, max(1, W - 8))
                f[y:y + rng.integers(1, 16), x:x + rng.integers(1, 8)] = rng.integers(0, 256, size=3, dtype=np.uint8)
        else:
            at = outlier_pixel(kind, npx)
            if kind in SINGLE:
                px = np.full(npx, SINGLE[kind], np.uint8)
            elif kind in ("steps_zero", "steps_z15"):
                px = _two_levels(rng, npx, 155, 255, at)
            else:
                px = _two_levels(rng, npx, 0, 100, at)
            px[at] = 0 if kind in ("onezero", "steps_zero", "steps_z15") else 255
            f = np.repeat(px.reshape(H, W, 1), 3, axis=2)
        out[i, :, :, :3] = f
        if C == 4:
            out[i, :, :, 3] = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    return out


Case = collections.namedtuple("Case", "rgb3 rgb4 planes")

@functools.lru_cache(maxsize=None)
def grey_lut():
    """ff.rgb2gray of the 256 grey pixels (v, v, v)."""
    lut = ff.rgb2gray(np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2))[:, 0]
    lut.setflags(write=False)
    return lut


def _plane(frame, kind):
    """ff.preprocess_u8(frame).  The oracle's grey product is a Python call per pixel; it is a function of the pixel's colour
    alone, so for the kinds with few colours it is taken once per colour (the CPU file holds planes of those kinds to
    ff.preprocess_u8 itself)."""
    if kind == "uniform":
        return ff.preprocess_u8(frame)
    colours, inverse = np.unique(frame.reshape(-1, 3), axis=0, return_inverse=True)
    gray = ff.rgb2gray(colours[None])[0][inverse.reshape(-1)].reshape(frame.shape[:2])
    return ff.pil_bilinear_u8(ff.bytescale(gray), IMG, IMG)


@functools.lru_cache(maxsize=None)
def case(H, W):
    """The frames of a geometry with 3 and with 4 channels (the same r, g, b; a random alpha byte) and the oracle's plane of
    each: computed once, shared by every test, read-only."""
    rng = np.random.default_rng(1000 * H + W)
    rgb4 = frames(rng, H, W, 4)
    rgb3 = np.ascontiguousarray(rgb4[..., :3])
    planes = np.stack([_plane(f, kind) for f, kind in zip(rgb3, KINDS)])
    for t in (rgb3, rgb4, planes):
        t.setflags(write=False)
    return Case(rgb3, rgb4, planes)


def first_difference(got, want):
    """(frame, y, x) of the first differing byte of two [n, 84, 84] plane arrays, with both values, or None."""
    d = np.argwhere(got != want)
    if d.size == 0:
        return None
    f, y, x = (int(v) for v in d[0])
    return "%d bytes differ, first at frame %d (%s) y %d x %d: got %d, want %d" % (
        len(d), f, KINDS[f] if f < len(KINDS) else "?", y, x, got[f, y, x], want[f, y, x])


# ---------------------------------------------------------------- plane history
HIST_AGENTS, HIST_PUSHES, HIST_DEPTH = 16, 19, 16
HIST_SIZES = (1, 74, 75, 192, 193, 208)
HIST_TRAIN_SIZE = 193
STACK = 4


def gather_trips(B, nout=IMG * IMG):
    """Trips of gather_history_kernel's grid-stride loop at B rows: work items / (grid x 256 threads), the grid capped."""
    total = B * (nout // 4)
    blocks = min((total + 255) // 256, GATHER_MAX_BLOCKS)
    return -(-total // (blocks * 256)), blocks


@functools.lru_cache(maxsize=None)
def history_planes():
    """[HIST_PUSHES, HIST_AGENTS, 84, 84, 1] random ready-made planes, push by push."""
    p = np.random.default_rng(77).integers(0, 256, size=(HIST_PUSHES, HIST_AGENTS, IMG, IMG, 1), dtype=np.uint8)
    p.setflags(write=False)
    return p


def history_live():
    """Every (agent, seq) whose four planes the ring still holds after the last push: pushed - (seq - 3) <= depth."""
    return [(a, s) for a in range(HIST_AGENTS) for s in range(STACK - 1, HIST_PUSHES) if HIST_PUSHES - (s - (STACK - 1)) <= HIST_DEPTH]


def history_state(agent, seq):
    """The [84, 84, 4] state whose newest plane is `seq` of `agent`: planes seq-3 .. seq, oldest first."""
    p = history_planes()
    return np.ascontiguousarray(np.stack([p[seq - STACK + 1 + c, agent, :, :, 0] for c in range(STACK)], axis=2))


def wraps(seq):
    """The four planes seq-3 .. seq sit in ring slots that wrap around the ring's end."""
    return seq >= HIST_DEPTH and seq % HIST_DEPTH < STACK - 1


@functools.lru_cache(maxsize=None)
def history_batch(B):
    """The first B names of a permutation of history_live().  From 75 rows on the last four rows -- rows of the grid's
    second trip -- are made to be: a name whose planes wrap the ring (and are not the newest), the oldest admissible plane of
    an agent, the newest of an agent, and row 0's name again."""
    live = history_live()
    rng = np.random.default_rng(500 + B)
    names = [live[i] for i in rng.permutation(len(live))[:B]]
    if B >= 75:
        oldest, newest = HIST_PUSHES - HIST_DEPTH + STACK - 1, HIST_PUSHES - 1
        names[B - 4] = (int(rng.integers(0, HIST_AGENTS)), HIST_DEPTH)          # seq 16: slots 13, 14, 15, 0
        names[B - 3] = (int(rng.integers(0, HIST_AGENTS)), oldest)
        names[B - 2] = (int(rng.integers(0, HIST_AGENTS)), newest)
        names[B - 1] = names[0]
    return tuple(names)

"""The crafted classify cases: one seeded 160 x 120 clip and tracks whose rectangles are chosen, not tracked -- the
geometries, limits and clip-at-zero situations that two recordings and a blob synthesiser do not produce.  Shared by
tests/golden/make_golden_classify_crafted.py (which runs the reference on them), tests/test_oracle_golden.py and
tests/test_classify_crafted_gpu.py, so that all three see the same cases and the same coverage assertion.

Everything here is plain integer arithmetic on the case list; nothing depends on what a kernel or the oracle gives."""
import numpy as np

W, H, T = 160, 120, 40
CROP = (1, 1, W - 2, H - 2)          # the clip's crop_rectangle (edge_pixels = 1)
SEED = 20250917
TIME_ON = [100000 + 111 * i for i in range(T)]
LAST_FFC = [40000] * T               # no frame is FFC-affected

# (variant name, hyper-parameters besides frame_size): the default model and the eight of
# tests/golden/make_golden_classify_variants.py
VARIANTS = {
    "default": {},
    "thermal_diff_norm": {"thermal_diff_norm": True},
    "no_diff_norm": {"diff_norm": False},
    "thermal_diff_norm_no_diff_norm": {"thermal_diff_norm": True, "diff_norm": False},
    "channels_swapped": {"channels": ["filtered", "thermal"]},
    "single_frame": {"square_width": 1},
    "single_frame_thermal_diff_norm": {"square_width": 1, "thermal_diff_norm": True},
    "inceptionv3_scaling": {"model_name": "inceptionv3"},
    "inceptionv3_scaling_single_frame": {"model_name": "inceptionv3", "square_width": 1},
}
# every variant at 32 and 64; the default also at 48 (a scale that is no power of two) and at 96 and 128 (two float32
# tiles above 64 KB of LDS); single_frame at 96 and 128 is the square_width 1 launch at those sizes
RUNS = [(v, fs) for fs in (32, 64) for v in VARIANTS] + [("default", 48), ("default", 96), ("default", 128),
                                                         ("single_frame", 96), ("single_frame", 128)]
FRAME_SIZES = (32, 48, 64, 96, 128)


def run_key(variant, fs):
    return "%s_fs%d" % (variant, fs)


class Region:
    """What the tests need of a track region (the reference's own Region is built from the same tuple)."""

    def __init__(self, frame_number, x, y, width, height, blank=False):
        self.frame_number, self.x, self.y, self.width, self.height, self.blank = frame_number, x, y, width, height, blank
        self.mass = width * height

    def as_tuple(self):
        return (self.frame_number, self.x, self.y, self.width, self.height, self.blank)


def clip_frames():
    """uint16 [T, H, W]: a smooth textured background with per-frame noise, a wide warm plateau and a cold patch that
    drift slowly (crops wholly above / below the frame median) and three small patches that move (filtered contrast)."""
    from cpx import synth

    rng = np.random.default_rng(SEED)
    frames = 2900.0 + 40.0 * synth.smooth_noise(rng, H, W)[None] + rng.normal(0.0, 4.0, size=(T, H, W))
    for t in range(T):
        px, _ = plateau(t)
        frames[t, 35:85, px:px + 64] += 300.0
        cx, _ = cold_patch(t)
        frames[t, 10:40, cx:cx + 30] -= 250.0
        frames[t, 90:100, 10 + 2 * t:22 + 2 * t] += 200.0       # warm, left to right
        frames[t, 100:112, 130 - 3 * t // 2:140 - 3 * t // 2] -= 120.0  # cold, right to left
        frames[t, 5 + t:13 + t, 80:90] += 150.0                   # warm, downwards
    return np.clip(np.rint(frames), 0, 65535).astype(np.uint16)


def plateau(t):
    return 40 + t // 2, 35      # x, y of the 64 x 50 warm plateau at frame t


def cold_patch(t):
    return 120 - t // 2, 10     # x, y of the 30 x 30 cold patch at frame t


def _place(w, h, where):
    """(x, y) of a w x h rectangle: 'c' centred (off every edge where the size allows), 'l' / 'r' / 't' / 'b' against
    that edge, 'L' / 'R' / 'T' / 'B' one pixel off it (still inside resize_and_pad's edge tests: the crop rectangle
    starts at 1 and ends at 159 / 119)."""
    x, y = (W - w) // 2, (H - h) // 2
    if where == "l":
        x = 0
    elif where == "L":
        x = min(1, W - w)
    elif where == "r":
        x = W - w
    elif where == "R":
        x = max(W - w - 1, 0)
    elif where == "t":
        y = 0
    elif where == "T":
        y = min(1, H - h)
    elif where == "b":
        y = H - h
    elif where == "B":
        y = max(H - h - 1, 0)
    elif where == "lt":
        x, y = 0, 0
    elif where == "rb":
        x, y = W - w, H - h
    else:
        assert where == "c", where
    return x, y


# (w, h, placement): the same list at every frame size; coverage() says which classes a size needs of it
GEOMETRIES = [
    # a single source pixel or line, upscaled
    (1, 1, "c"), (1, 7, "c"), (7, 1, "c"), (2, 2, "c"), (1, 1, "lt"), (1, 7, "r"), (7, 1, "b"), (2, 2, "rb"),
    # exactly fs, fs - 1, fs + 1 (square where the 120 lines allow, else 60 high: the x axis alone)
    (31, 31, "c"), (32, 32, "c"), (33, 33, "c"), (47, 47, "c"), (48, 48, "c"), (49, 49, "c"),
    (63, 63, "c"), (64, 64, "c"), (65, 65, "c"), (95, 95, "c"), (96, 96, "c"), (97, 97, "c"),
    (127, 60, "c"), (128, 60, "c"), (129, 60, "c"), (31, 33, "c"), (65, 63, "c"),
    # the whole frame, and both opposite edges at once (the first test, left / top, wins)
    (160, 120, "c"), (160, 30, "c"), (150, 120, "c"), (100, 120, "l"),
    # round() on an exact half: 2.5 -> 2 and 3.5 -> 4 (fs 32 and 64 with 64 / 128 long, fs 48 with 96 long), 1.5 -> 2
    # (128 x 6 at fs 32, 128 x 2 at fs 96), 4.5 -> 4 (128 x 6 at fs 96)
    (5, 64, "c"), (7, 64, "c"), (64, 5, "c"), (64, 7, "c"), (128, 6, "c"), (128, 10, "c"), (128, 5, "c"), (128, 7, "c"),
    (96, 5, "c"), (96, 7, "c"), (5, 96, "c"), (7, 96, "c"), (5, 64, "r"), (64, 7, "b"), (128, 5, "T"), (7, 96, "L"),
    # the short side rounds to 0 and is clamped to 1
    (128, 2, "c"), (128, 1, "c"), (128, 1, "b"), (1, 120, "c"), (1, 120, "r"), (160, 1, "c"),
    # placement with the resized side shorter than fs: against each edge, one pixel off it, and centred
    (20, 60, "l"), (20, 60, "L"), (20, 60, "r"), (20, 60, "R"), (20, 60, "c"), (60, 20, "t"), (60, 20, "T"),
    (60, 20, "b"), (60, 20, "B"), (60, 20, "c"), (20, 30, "lt"), (30, 20, "rb"), (13, 9, "c"), (9, 13, "c"),
    (40, 27, "c"), (27, 40, "c"),
    # more of the first classes in other places, and one pixel short of the whole frame
    (1, 1, "rb"), (2, 2, "lt"), (1, 7, "T"), (7, 1, "R"), (33, 31, "c"), (63, 65, "c"), (159, 119, "c"), (158, 118, "c"),
]
assert len(GEOMETRIES) == 75  # three 25-frame segments, one geometry per frame


def tracks():
    """-> list of dict(name, regions [Region], segments [[frame number] * 25]).  Track i has id i + 1 and starts at
    frame 0; its regions are on consecutive frames."""
    out = []
    for g in range(3):  # 75 geometries, 25 per track, one segment each
        regions = []
        for t in range(25):
            w, h, where = GEOMETRIES[25 * g + t]
            x, y = _place(w, h, where)
            regions.append(Region(t, x, y, w, h))
        out.append(dict(name="geometry%d" % g, regions=regions, segments=[list(range(25))]))
    # clip_thermals_at_zero: every sampled crop inside the warm plateau (stays on) ...
    warm = [Region(t, plateau(t)[0] + 4, 40, 20 + t % 5, 24) for t in range(25)]
    out.append(dict(name="clip_on", regions=warm, segments=[list(range(25))]))
    # ... and the same with one crop inside the cold patch (goes off for the whole track)
    mixed = [Region(t, plateau(t)[0] + 4, 40, 20 + t % 5, 24) for t in range(25)]
    mixed[12] = Region(12, cold_patch(12)[0] + 4, 14, 12, 12)
    out.append(dict(name="clip_off", regions=mixed, segments=[list(range(25))]))
    # limits: 1, 16, 17 and 40 usable regions (the limits kernel deals a track's regions to 16 waves), with blank
    # regions and regions of zero width / height in between, which are skipped
    one = [Region(t, 30 + t, 88, 14, 14, blank=(t != 3)) for t in range(10)]
    out.append(dict(name="limits1", regions=one, segments=[[3] * 25]))
    for n in (16, 17):
        regs = [Region(t, 8 + 2 * t, 86, 16, 16) for t in range(n)]
        regs += [Region(n, 60, 60, 10, 10, blank=True), Region(n + 1, 60, 60, 0, 10), Region(n + 2, 60, 60, 10, 0),
                 Region(n + 3, 20, 90, 12, 12, blank=True)]
        out.append(dict(name="limits%d" % n, regions=regs, segments=[sorted(i * n // 25 for i in range(25))]))
    forty = [Region(t, 125 - 3 * t // 2, 98, 16, 16) if t % 2 else Region(t, 6 + 2 * t, 86, 18, 16) for t in range(T)]
    out.append(dict(name="limits40", regions=forty, segments=[sorted(list(range(0, 40, 2)) + [1, 9, 17, 25, 33])]))
    for t in out:
        for seg in t["segments"]:
            assert len(seg) == 25 and seg == sorted(seg)
        for i, r in enumerate(t["regions"]):
            assert r.frame_number == i < T
            assert 0 <= r.x and r.x + r.width <= W and 0 <= r.y and r.y + r.height <= H, (t["name"], r.as_tuple())
    return out


def usable(regions):
    return [r for r in regions if not r.blank and r.width > 0 and r.height > 0]


def resized(w, h, fs):
    """(dw, dh, half-way flags, clamped flags) of resize_and_pad's round(side * scale) in exact integer arithmetic:
    scale = fs / max(w, h), so side * scale = side * fs / long."""
    long = max(w, h)
    out = []
    for side in (w, h):
        q, r = divmod(2 * side * fs, long)          # 2 * side * scale = q + r / long
        half = r == 0 and q % 2 == 1
        n = q // 2                                   # floor(side * scale)
        if half:
            rounded = n if n % 2 == 0 else n + 1     # to even
        else:
            rounded = n + (1 if (q % 2 == 1) else 0)  # above a half (q odd, r > 0) rounds up; q even rounds down
        out.append((min(max(rounded, 1), fs), half, n % 2 == 0 if half else None, rounded == 0))
    return out


def coverage(fs, track_list):
    """Assert that the case list hits every geometry class at frame size fs (both axes where the frame allows it), and
    return the set of classes hit."""
    hit = set()
    for t in track_list:
        sampled = {f for s in t["segments"] for f in s}
        for r in usable(t["regions"]):
            if r.frame_number not in sampled:
                continue
            w, h = r.width, r.height
            (dw, half_x, down_x, zero_x), (dh, half_y, down_y, zero_y) = resized(w, h, fs)
            if (w, h) in ((1, 1), (1, 7), (7, 1), (2, 2)):
                hit.add("tiny%dx%d" % (w, h))
            for d, tag in ((-1, "fs-1"), (0, "fs"), (1, "fs+1")):
                if w == fs + d:
                    hit.add("x" + tag)
                if h == fs + d:
                    hit.add("y" + tag)
            if (w, h) == (W, H):
                hit.add("whole")
            if half_x:
                hit.add("half_x_down" if down_x else "half_x_up")
            if half_y:
                hit.add("half_y_down" if down_y else "half_y_up")
            if zero_x:
                hit.add("clamp_x")
            if zero_y:
                hit.add("clamp_y")
            left, right = r.x <= CROP[0], r.x + w >= CROP[0] + CROP[2]
            top, bottom = r.y <= CROP[1], r.y + h >= CROP[1] + CROP[3]
            if dw < fs:
                hit.update((["left"] if left and not right else []) + (["right"] if right and not left else [])
                           + (["both_x"] if left and right else []) + (["centre_x"] if not left and not right else []))
            if dh < fs:
                hit.update((["top"] if top and not bottom else []) + (["bottom"] if bottom and not top else [])
                           + (["both_y"] if top and bottom else []) + (["centre_y"] if not top and not bottom else []))
            if r.x == 0 and w == W:
                hit.add("full_width")
    need = {"tiny1x1", "tiny1x7", "tiny7x1", "tiny2x2", "xfs-1", "xfs", "xfs+1", "whole", "left", "right", "top",
            "bottom", "centre_x", "centre_y", "both_y", "full_width"}
    if fs + 1 <= H:
        need |= {"yfs-1", "yfs", "yfs+1"}          # at fs 128 a region fs high does not fit the 120 lines
    # side * fs / long is an exact half only when long / gcd(long, 2 fs) ... in this frame: long 64 or 128 at fs 32,
    # 128 at fs 64 (x only: 128 lines do not exist), 96 at fs 48, 128 at fs 96 (x only); none at fs 128 (long would
    # have to be a multiple of 256)
    need |= {32: {"half_x_down", "half_x_up", "half_y_down", "half_y_up"}, 48: {"half_x_down", "half_x_up", "half_y_down",
             "half_y_up"}, 64: {"half_y_down", "half_y_up"}, 96: {"half_y_down", "half_y_up"}, 128: set()}[fs]
    # a side of 1 rounds to 0 only below fs / long = 0.5: long 128 or 160 up to fs 64 (the y side), long 120 up to fs 48
    need |= {32: {"clamp_x", "clamp_y"}, 48: {"clamp_x", "clamp_y"}, 64: {"clamp_y"}, 96: set(), 128: set()}[fs]
    assert need <= hit, (fs, sorted(need - hit))
    usable_counts = sorted(len(usable(t["regions"])) for t in track_list if t["name"].startswith("limits"))
    assert usable_counts == [1, 16, 17, 40]
    assert any(r.blank for t in track_list for r in t["regions"])
    assert any(r.width == 0 for t in track_list for r in t["regions"])
    assert any(r.height == 0 for t in track_list for r in t["regions"])
    return hit


def clip_at_zero_expected(frames, track):
    """The reference's test (interpreter.py:391-399) on the sampled crops, with integers: the crop's median against the
    frame's.  2 * median is an integer for both (a median of integers is k / 2)."""
    clip = True
    for fn in sorted({f for s in track["segments"] for f in s}):
        r = track["regions"][fn]
        crop2 = int(round(2 * float(np.median(frames[fn][r.y:r.y + r.height, r.x:r.x + r.width]))))
        frame2 = int(round(2 * float(np.median(frames[fn]))))
        if crop2 <= frame2:
            clip = False
    return clip

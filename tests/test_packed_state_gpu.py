"""The packed background state (cpx_frame_kernel<true>): a fresh batch of at most 1023 processed
frames per clip (window <= 64) keeps the per-pixel count of consecutive kept frames in the top ten bits of the window
sum, and every path that continues from that state or exports it unpacks it first (cpx_api.cpp: unpack_state) -- a
CPX_TRACK_KEEP_BACKGROUND call, a resumed cpx_track_frame stream, cpx_get_background.

Pinned here against the oracle (oracle/track_oracle.py, the reference's WeightedBackground.process_frame,
piclassifier/motiondetector.py:197-237) and against the two-array kernel (CPX_TRACK_PACKED_STATE=0): the exported
weights of every clip, the 1023 / 1024 switch with the largest count and window sum the packed word holds, the
hand-offs to a KEEP call and to a resumed stream, the launch forms, and the handle's bookkeeping of that state.
Weights are compared exactly: the device table is the same repeated float64 addition as NumPy's."""
import types

import numpy as np
import pytest

from helpers import crc

pytestmark = pytest.mark.gpu

H, W, E = 120, 160, 1
ENV = ("CPX_TRACK_PACKED_STATE", "CPX_TRACK_PER_STEP")
INFO_FIELDS = ("frame_number", "n_components", "status", "ffc_affected", "avg_change", "norm_min", "norm_max",
               "threshold", "filt_min", "filt_max", "thermal_min", "thermal_max", "thermal_sum", "thermal_median",
               "filtered_abs_sum", "background_average", "background_changed")

# staircase: a flat background L, patches held at L + D from the first processed frame on.  With weight_add 0.1 a patch
# is released (background := frame, weight := 0) after about 10 D kept frames: at 10, 290 / 310 (both sides of a resume
# after 300), 500 / 520 (both sides of the LDS weight table's 512 entries), 600, 801, 1011 / 1021 / 1031 / 1051 (both
# sides of 1023 / 1024).  w_520 = 52.00000000000047 and w_800 = 79.99999999999973 lie within 1e-6 of f - bg: those
# decisions take the float64 expression from the global table (cpx_track.hip, streaming pass) while the state is packed.
STAIR_L = 3000
STAIR_D = (1, 29, 31, 50, 52, 60, 80, 101, 102, 103, 105)


def staircase(n_proc):
    """frames [n_proc + 1, H, W] (frame 0: the background, flagged), background flags."""
    f = np.full((n_proc + 1, H, W), STAIR_L, np.uint16)
    for i, d in enumerate(STAIR_D):
        r, c = divmod(i, 4)
        y, x = 8 + r * 36, 8 + c * 38
        f[1:, y:y + 12, x:x + 14] = STAIR_L + d
    return f, [True] + [False] * n_proc


def synth_clip(rng, n, model="lepton3"):
    """A synthetic clip with a leading background frame, one in the middle and FFC-affected frames."""
    from cpx import synth

    frames = synth.make_clip(rng, n, model=model)
    t_on, ffc = synth.frame_times(n)
    bgf = [False] * n
    if n >= 3:
        bgf[0] = True
    if n >= 40:
        bgf[n // 3] = True
        for i in range(n // 2, n // 2 + 3):
            ffc[i] = t_on[i] - 5
    return frames, t_on, ffc, bgf


class Oracle:
    """Compact per-frame record of track_oracle.track_clip (do_tracking=False) and its background state after the
    processed frames in `states` (default: the last one)."""

    def __init__(self, frames, model="lepton3", t_on=None, ffc=None, bgf=None, window=45, background=None,
                 states=None):
        import track_oracle as to

        cfg = to.OracleConfig(model)
        cfg.window = window
        self.weight_add = cfg.weight_add
        out = to.track_clip(frames, t_on, ffc, bgf, cfg, keep=True, do_tracking=False, background=background)
        recs = out["frames"]
        self.n = len(recs)
        self.avg_change = np.array([o["avg_change"] for o in recs])
        self.threshold = np.array([np.float32(o["threshold"]) for o in recs])
        self.norm_min = np.array([int(o["norm_min"]) for o in recs])
        self.norm_max = np.array([int(o["norm_max"]) for o in recs])
        self.bg_avg = np.array([o["bg_after_avg"] for o in recs])
        self.n_components = np.array([o["n_components"] for o in recs])
        self.ffc = np.array([bool(o["ffc"]) for o in recs])
        self.crc_filt = [crc(o["filtered"].astype(np.int32)) for o in recs]
        self.crc_mask = [crc(o["mask"].astype(np.int32)) for o in recs]
        want = set(states if states is not None else []) | {self.n - 1}
        self.states = {q: (recs[q]["bg_after"].astype(np.float64), recs[q]["weight_after"].copy(), recs[q]["bg_after_avg"])
                       for q in want if 0 <= q < self.n}

    def state(self, q=-1):
        return self.states[self.n - 1 if q == -1 else q]

    def model(self, q=-1):
        """The state after processed frame q as a WeightedBackground to continue from."""
        import track_oracle as to

        bg, w, avg = self.state(q)
        wb = to.WeightedBackground(W, H, self.weight_add, E)
        wb.background, wb.weight, wb.average = bg.copy(), w.copy(), avg
        return wb


def check_frames(info, labels, filt, f0, bgf, orc, q0=0, n_proc=None):
    """Per-frame records of one clip (frames f0 .. f0 + len(bgf)) against oracle frames q0 .. q0 + n_proc."""
    proc = [f0 + i for i in range(len(bgf)) if not bgf[i]]
    skip = [f0 + i for i in range(len(bgf)) if bgf[i]]
    n_proc = len(proc) if n_proc is None else n_proc
    proc = proc[:n_proc]
    assert (info["frame_number"][skip] == -1).all()
    fi = info[proc]
    q = np.arange(q0, q0 + len(proc))
    assert np.array_equal(fi["frame_number"], q)
    for name, want in (("avg_change", orc.avg_change), ("threshold", orc.threshold), ("norm_min", orc.norm_min),
                       ("norm_max", orc.norm_max), ("background_average", orc.bg_avg),
                       ("n_components", orc.n_components), ("ffc_affected", orc.ffc.astype(np.int32))):
        bad = np.nonzero(fi[name] != want[q])[0]
        assert bad.size == 0, (name, int(q[bad[0]]))
    for j, f in enumerate(proc):
        if filt is not None:
            assert crc(filt[f].astype(np.int32)) == orc.crc_filt[q[j]], ("filtered", int(q[j]))
        if labels is not None:
            assert crc(labels[f]) == orc.crc_mask[q[j]], ("labels", int(q[j]))
    return len(proc)


def check_state(got, want, what=""):
    bg, w, avg = got
    wbg, ww, wavg = want
    assert np.array_equal(bg.astype(np.float64), wbg), ("background", what)   # edges replicated on both sides
    bad = np.argwhere(w != ww)
    assert bad.size == 0, ("weights", what, tuple(bad[0]), w[tuple(bad[0])], ww[tuple(bad[0])])
    assert avg == float(wavg), ("average", what, avg, wavg)


def make_engine(monkeypatch, packed=None, per_step=None, **kw):
    """A TrackEngine whose handle reads the given launch / state switches (read at cpx_create)."""
    from cpx.engine import TrackEngine

    for name, v in zip(ENV, (packed, per_step)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    eng = TrackEngine(model=kw.pop("model", "lepton3"), **kw)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return eng


def batch(clips, eng):
    """[(frames, t_on, ffc, bgf)] -> device frames, offsets, meta."""
    offs, metas = [0], []
    for fr, t_on, ffc, bgf in clips:
        metas.append(eng.make_meta(fr.shape[0], t_on, ffc, bgf))
        offs.append(offs[-1] + fr.shape[0])
    return (eng.upload_frames(np.concatenate([c[0] for c in clips])), np.array(offs, np.int32),
            np.concatenate(metas))


def stair_clip(n_proc):
    fr, bgf = staircase(n_proc)
    return fr, None, None, bgf


def get_all(eng, B):
    return [eng.get_background(b) for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------------
# oracle runs shared by the tests (the host oracle costs about 2 ms per frame)
# ---------------------------------------------------------------------------------------------------------------------
STAIR_LONG = 1100          # processed frames of the long staircase; its first 1023 / 1024 are the packed / unpacked prefixes
SYN_LENS = (1, 40, 97, 250)


@pytest.fixture(scope="module")
def stair_oracle():
    fr, bgf = staircase(STAIR_LONG)
    return Oracle(fr, "lepton3", bgf=bgf, states=(0, 299, 300, 1022, 1023))


def _synth_set(model, seed, lens=SYN_LENS):
    rng = np.random.default_rng(seed)
    return [synth_clip(rng, n, model) for n in lens]


def _flags():
    from cpx import _lib

    return dict(none=0, freeze_ffc=_lib.TRACK_FREEZE_ON_FFC, freeze_bg=_lib.TRACK_FREEZE_BACKGROUND,
                defer=_lib.TRACK_DEFER_MEDIANS)


# ---------------------------------------------------------------------------------------------------------------------
# 1. packed == two arrays, under every launch form
# ---------------------------------------------------------------------------------------------------------------------
FORMS = [("fused", "none"), ("fused", "freeze_ffc"), ("fused", "freeze_bg"), ("fused", "defer"), ("per_step", "none"),
         ("denoise", "none")]


@pytest.mark.parametrize("form,flag", FORMS)
def test_packed_equals_two_array_state(monkeypatch, form, flag):
    if form == "denoise":   # (short: two NLM launches per step)
        clips = _synth_set("lepton3", 21, (1, 14, 30)) + [stair_clip(60)]
    else:
        clips = _synth_set("lepton3", 20) + [stair_clip(1023)]
    B = len(clips)
    want_filtered = form != "per_step"   # (per step: the workspace layout with the filtered ping-pong inside)
    outs = []
    for packed in (0, 1):
        eng = make_engine(monkeypatch, packed=packed, per_step=1 if form == "per_step" else None, denoise=form == "denoise")
        dev, offs, meta = batch(clips, eng)
        res = eng.track_batch(dev, offs, meta, want_labels=True, want_filtered=want_filtered, want_background=True,
                              flags=_flags()[flag])
        res.check()
        total = int(offs[-1])
        outs.append(dict(info=res.info.copy(), comps=[res.components(f).copy() for f in range(total)],
                         labels=res.labels(), filtered=res.filtered(), background=res.background(),
                         state=get_all(eng, B)))
        del res
        eng.close()
    a, b = outs
    assert a["info"].tobytes() == b["info"].tobytes()
    for f, (x, y) in enumerate(zip(a["comps"], b["comps"])):
        assert x.tobytes() == y.tobytes(), f
    assert sum(len(c) for c in a["comps"]) > 0
    assert np.array_equal(a["labels"], b["labels"])
    if want_filtered:
        assert a["filtered"].tobytes() == b["filtered"].tobytes()
    assert a["background"].tobytes() == b["background"].tobytes()
    for c in range(B):
        (bg0, w0, avg0), (bg1, w1, avg1) = a["state"][c], b["state"][c]
        assert bg0.tobytes() == bg1.tobytes() and w0.tobytes() == w1.tobytes() and avg0 == avg1, c
    if form != "denoise" and flag != "freeze_bg":
        assert a["state"][-1][1].max() > 100.0   # (the staircase's last patch: counted to the packed word's limit)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the exported state of a packed batch against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["lepton3", "lepton3.5"])
def test_packed_state_matches_oracle(monkeypatch, stair_oracle, model):
    clips = _synth_set(model, 30 if model == "lepton3" else 35) + [stair_clip(1023)]
    eng = make_engine(monkeypatch, model=model)
    dev, offs, meta = batch(clips, eng)
    res = eng.track_batch(dev, offs, meta, want_labels=True, want_filtered=True, want_background=True)
    res.check()
    info, labels, filt, bgs = res.info, res.labels(), res.filtered(), res.background()
    for b, (fr, t_on, ffc, bgf) in enumerate(clips):
        if b == len(clips) - 1 and model == "lepton3":
            orc, q = stair_oracle, 1022
        else:
            orc, q = Oracle(fr, model, t_on, ffc, bgf), -1
        n = check_frames(info, labels, filt, int(offs[b]), bgf, orc, n_proc=orc.n if q == -1 else q + 1)
        assert n == (orc.n if q == -1 else q + 1)
        want = orc.state(q)
        assert np.array_equal(bgs[b].astype(np.float64), want[0]), b
        check_state(eng.get_background(b), want, (model, b))
    if model == "lepton3":
        w = eng.get_background(len(clips) - 1)[1]
        assert w.max() == stair_oracle.state(1022)[1].max() > 102.0   # 1023 kept frames: the ten-bit count's largest
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the count-width boundary: 1023 processed frames (packed) / 1024 (two arrays by rule), window 64
# ---------------------------------------------------------------------------------------------------------------------
def _saturated_clip(n_proc):
    """Frame 0 (flagged background) low everywhere; then a block at 65535 that stays kept on every frame: after 64 frames
    its window sum is 64 x 65535 = 4,194,240, the largest the packed word's 22 bits hold."""
    f = np.full((n_proc + 1, H, W), 100, np.uint16)
    f[1:, 40:60, 50:90] = 65535
    return f, None, None, [True] + [False] * n_proc


def test_count_width_boundary(monkeypatch):
    wa = 0.1
    acc = np.zeros(1025)
    for k in range(1, acc.size):
        acc[k] = acc[k - 1] + wa
    c23, c24 = _saturated_clip(1023), _saturated_clip(1024)
    orc = Oracle(c24[0], "lepton3", bgf=c24[3], window=64, states=(1022, 1023))
    runs = {}
    for name, clips, packed in (("1023", [c23], None), ("1024", [c24], None), ("both", [c23, c24], None),
                                ("1023-two-arrays", [c23], 0)):
        eng = make_engine(monkeypatch, packed=packed, window=64)
        dev, offs, meta = batch(clips, eng)
        res = eng.track_batch(dev, offs, meta, want_labels=True, want_filtered=True)
        res.check()
        info, labels, filt = res.info, res.labels(), res.filtered()
        states = []
        for b, c in enumerate(clips):
            n = len(c[3]) - 1
            check_frames(info, labels, filt, int(offs[b]), c[3], orc)
            st = eng.get_background(b)
            check_state(st, orc.state(n - 1), (name, b))
            block = np.zeros(st[1].shape, bool)
            block[39:59, 49:89] = True                                   # (the block in interior coordinates)
            assert (st[1][block] == acc[n]).all() and (st[1][~block] == 0).all(), (name, b)
            states.append(st)
        runs[name] = (info.copy(), labels, filt, states)
        del res
        eng.close()
    a, b = runs["1023"], runs["1023-two-arrays"]
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()
    assert a[3][0][1].tobytes() == b[3][0][1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a stream resumed after a packed prefix (TrackStream.replay: the extractor's capacity regrow)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resume_clips(stair_oracle):
    rng = np.random.default_rng(44)
    fr, t_on, ffc, bgf = synth_clip(rng, STAIR_LONG + 1)
    bgf[1060] = True                       # (one more background frame past the last split point)
    syn = ((fr, t_on, ffc, bgf), Oracle(fr, "lepton3", t_on, ffc, bgf))
    return [(stair_clip(STAIR_LONG), stair_oracle), syn]


@pytest.mark.parametrize("k", [1, 300, 1023, 1024])
def test_resume_after_packed_prefix(monkeypatch, resume_clips, k):
    eng = make_engine(monkeypatch)
    for c, ((fr, t_on, ffc, bgf), orc) in enumerate(resume_clips):
        n = fr.shape[0]
        meta = eng.make_meta(n, t_on, ffc, bgf)
        dev = eng.upload_frames(fr)
        whole = eng.track_batch(dev, np.array([0, n], np.int32), meta, want_labels=True, want_filtered=True)
        whole.check()
        w_info, w_labels, w_filt = whole.info.copy(), whole.labels(), whole.filtered()
        w_state = eng.get_background(0)
        del whole
        # the first `consumed` frames hold k processed ones; the old stream stood there
        consumed = int(np.nonzero(np.cumsum(~np.asarray(bgf)) == k)[0][0]) + 1
        old = types.SimpleNamespace(n=consumed, frames_dev=dev, meta=meta)
        s = eng.open_stream(n, want_labels=True)
        s.replay(old, associate=False)
        for i in range(consumed, n):
            s.append(fr[i], None if t_on is None else t_on[i], None if ffc is None else ffc[i], init_only=bgf[i],
                     associate=False)
        res = s.result
        info, labels, filt = res.info, res.labels(), res.filtered()
        assert check_frames(info, labels, filt, 0, bgf, orc) == orc.n
        check_state(eng.get_background(0), orc.state(), (k, c))
        for name in INFO_FIELDS:   # (bytes: the records of background frames are all ones, NaN as floats)
            assert info[name].tobytes() == w_info[name].tobytes(), (k, c, name)
        proc = ~np.asarray(bgf)   # (images of background frames are never written: the two buffers' own contents)
        assert np.array_equal(labels[proc], w_labels[proc]) and filt[proc].tobytes() == w_filt[proc].tobytes(), (k, c)
        st = eng.get_background(0)
        assert st[0].tobytes() == w_state[0].tobytes() and st[1].tobytes() == w_state[1].tobytes() and st[2] == w_state[2]
        del s, res
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. CPX_TRACK_KEEP_BACKGROUND after a packed batch (clip 1 staged, clips 0 and 2 continue from the packed state)
# ---------------------------------------------------------------------------------------------------------------------
def test_keep_background_after_packed_batch(monkeypatch):
    from cpx import _lib

    rng = np.random.default_rng(55)
    first, second = [], []
    for n1, n2 in ((60, 50), (150, 80), (200, 120)):
        fr, t_on, ffc, bgf = synth_clip(rng, n1 + n2)
        first.append((fr[:n1], t_on[:n1], ffc[:n1], bgf[:n1]))
        bg2 = list(bgf[n1:])
        second.append((fr[n1:], t_on[n1:], ffc[n1:], bg2))
    orcs1 = [Oracle(fr, "lepton3", t_on, ffc, bgf, states=(40,)) for fr, t_on, ffc, bgf in first]
    staged = orcs1[1].state(40)           # clip 1: a state of its own past, not the one its first call left
    starts = [orcs1[0].model(), orcs1[1].model(40), orcs1[2].model()]
    orcs2 = [Oracle(c[0], "lepton3", c[1], c[2], c[3], background=wb) for c, wb in zip(second, starts)]
    runs = []
    for packed in (1, 0):
        eng = make_engine(monkeypatch, packed=packed)
        dev, offs, meta = batch(first, eng)
        r1 = eng.track_batch(dev, offs, meta, want_filtered=True)
        r1.check()
        eng.set_background(1, staged[0].astype(np.float32), staged[1], staged[2])
        dev, offs, meta = batch(second, eng)
        r2 = eng.track_batch(dev, offs, meta, want_labels=True, want_filtered=True, want_background=True,
                             flags=_lib.TRACK_KEEP_BACKGROUND)
        r2.check()
        info, labels, filt = r2.info, r2.labels(), r2.filtered()
        for b, c in enumerate(second):
            assert check_frames(info, labels, filt, int(offs[b]), c[3], orcs2[b]) == orcs2[b].n
            check_state(eng.get_background(b), orcs2[b].state(), (packed, b))
            assert np.array_equal(r2.background()[b].astype(np.float64), orcs2[b].state()[0])
        runs.append((info.copy(), labels, filt, get_all(eng, 3)))
        del r1, r2
        eng.close()
    a, b = runs
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()
    for x, y in zip(a[3], b[3]):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2]
    assert any(s[1].max() > 0 for s in a[3])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the handle's bookkeeping of the state across calls
# ---------------------------------------------------------------------------------------------------------------------
def test_state_bookkeeping_across_calls(monkeypatch, stair_oracle):
    from cpx import _lib
    from cpx._lib import CpxError

    eng = make_engine(monkeypatch)
    syn = _synth_set("lepton3", 66, (30, 80, 120))
    syn_orc = [Oracle(fr, "lepton3", t_on, ffc, bgf) for fr, t_on, ffc, bgf in syn]

    def packed_call(want_filtered):
        dev, offs, meta = batch(syn, eng)
        r = eng.track_batch(dev, offs, meta, want_labels=True, want_filtered=want_filtered)
        r.check()
        for b, c in enumerate(syn):
            check_frames(r.info, r.labels(), r.filtered(), int(offs[b]), c[3], syn_orc[b])
        return r

    # packed, B = 3: every clip's state, read twice (the second read must not unpack again)
    r = packed_call(True)
    s1, s2 = get_all(eng, 3), get_all(eng, 3)
    for b in range(3):
        check_state(s1[b], syn_orc[b].state(), ("first read", b))
        check_state(s2[b], syn_orc[b].state(), ("second read", b))
    # fresh, B = 2, a clip of 1024 processed frames: unpacked; nothing of the packed words may leak into it
    short = syn[0]
    dev, offs, meta = batch([stair_clip(1024), short], eng)
    r = eng.track_batch(dev, offs, meta, want_labels=True, want_filtered=True)
    r.check()
    check_frames(r.info, r.labels(), r.filtered(), 0, stair_clip(1024)[3], stair_oracle, n_proc=1024)
    check_frames(r.info, r.labels(), r.filtered(), int(offs[1]), short[3], syn_orc[0])
    check_state(eng.get_background(0), stair_oracle.state(1023), "unpacked 1024")
    check_state(eng.get_background(1), syn_orc[0].state(), "unpacked short")
    # packed, B = 3, no filtered output (the workspace layout with the filtered ping-pong)
    r = packed_call(False)
    # refused before the state is touched: KEEP with another batch size and nothing staged; a staged clip outside
    dev, offs, meta = batch(syn[:2], eng)
    with pytest.raises(CpxError) as ei:
        eng.track_batch(dev, offs, meta, flags=_lib.TRACK_KEEP_BACKGROUND)
    assert ei.value.code == -1
    bg, w, avg = syn_orc[0].state()
    eng.set_background(3, bg.astype(np.float32), w, avg)
    dev, offs, meta = batch(syn, eng)
    with pytest.raises(CpxError) as ei:
        eng.track_batch(dev, offs, meta)
    assert ei.value.code == -1
    for b in range(3):
        check_state(eng.get_background(b), syn_orc[b].state(), ("after refusals", b))
    del r
    assert eng.lib.cpx_release_memory(eng.h) == 0
    with pytest.raises(CpxError) as ei:
        eng.get_background(0)
    assert ei.value.code == -1
    eng.close()

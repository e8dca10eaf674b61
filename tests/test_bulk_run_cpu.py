"""The decisions of the file-fed driver (cpx/track/bulk.py) that need no device: the gzip trailer rule, the file table of an
inflate launch, a batch's bookkeeping and the order batches close in, the lane rules, and the order of the kept tracks
with their rows in the region pool -- host logic, no GPU."""
from concurrent.futures import Future

import numpy as np

from cpx.track import bulk
from cpx.tracking import REGION_DTYPE, TRACK_SUMMARY_DTYPE


def test_trailer_rule():
    assert bulk.trusted_isize(17, 5) == 0                             # shorter than a gzip member: no trailer
    assert bulk.trusted_isize(18, 5) == 5
    for size in (18, 1000, 1 << 20):
        assert bulk.trusted_isize(size, 1032 * size + 64) == 1032 * size + 64
        assert bulk.trusted_isize(size, 1032 * size + 65) == 0
    assert bulk.isize_limit(np.array([0, 17, 18, 100])).tolist() == [0, 0, 1032 * 18 + 64, 103264]


def test_file_table_layout():
    """Four files: a plain one, one already in error, one whose trailer claims MAX_INFLATED + 1 (refused), a plain one
    behind them -- the figures below from the formulas, by hand."""
    sizes = np.array([1000, 500, 2 << 20, 33], np.int64)
    in_off = bulk.staged_offsets(sizes)
    assert in_off.tolist() == [0, 1008, 1520, 1520 + (2 << 20), 1520 + (2 << 20) + 48]     # each rounded up to 16
    isize = np.array([100001, 7000, bulk.MAX_INFLATED + 1, 2500], np.int64)
    assert bulk.MAX_INFLATED + 1 <= 1032 * (2 << 20) + 64                                 # refused for its size alone
    files, out_off, slot_off, refused = bulk.file_table(sizes, in_off, isize, {1: "unreadable"}, min_pixels=160 * 120)
    assert refused == [2]
    assert files["in_offset"].tolist() == in_off[:-1].tolist()
    assert files["in_bytes"].tolist() == [1000, 0, 0, 33]
    assert files["out_capacity"].tolist() == [100001, 0, 0, 2500]
    # every file's output: its capacity rounded up to 16, + 16
    assert out_off.tolist() == [0, 100016 + 16, 100032 + 16, 100048 + 16, 100064 + 2512 + 16]
    assert files["out_offset"].tolist() == out_off[:-1].tolist()
    # the smallest frame section: 4 + a payload at one bit per delta (19,199 deltas -> 2,400 bytes) + 8
    min_frame = 4 + 2400 + 8
    assert files["slot_capacity"].tolist() == [100001 // min_frame + 1, 1, 1, 2500 // min_frame + 1] == [42, 1, 1, 2]
    assert slot_off.tolist() == [0, 42, 43, 44, 46] and files["slot_offset"].tolist() == [0, 42, 43, 44]
    # a smaller frame (the engine's resolution, as the inflate tests pass it): more slots for the same bytes
    files, _, slot_off, refused = bulk.file_table(sizes, in_off, isize, {}, min_pixels=32 * 24)
    assert files["slot_capacity"].tolist()[:2] == [100001 // (4 + 96 + 8) + 1, 7000 // 108 + 1] and refused == [2]
    # a trailer beyond what DEFLATE can expand the file to is refused as well
    assert bulk.file_table(sizes, in_off, np.array([1032 * 1000 + 65, 0, 0, 0]), {}, 160 * 120)[3] == [0]


def _done(value=None, error=None):
    f = Future()
    if error is not None:
        f.set_exception(error)
    else:
        f.set_result(value)
    return f


def test_batch_record_completes_and_closes_in_order():
    paths = ["a", "b", "c", "d"]
    batch = bulk.BatchRecord(paths, 0, {3: "d: not gzip"}, [[0, 1], [2]])
    assert batch.expected == {0, 1, 2} and batch.retry == {3: "d: not gzip"}
    batch.group_submitted()
    assert not batch.complete()
    batch.group_drained()
    assert not batch.complete()                  # the one submitted group drained: the last was not submitted yet
    batch.group_submitted()
    assert not batch.complete()                  # two groups, one drained
    batch.group_drained()
    assert batch.complete()
    assert bulk.BatchRecord(paths, 0, {}, []).complete()     # nothing decoded: complete at once

    first, second = bulk.BatchRecord(["a"], 0, {}, [[0]]), bulk.BatchRecord(["b"], 1, {}, [[0]])
    slow = Future()
    first.futures.append(slow)
    second.futures.append(_done(({0: "text b"}, {}, 10, 0.5)))
    closing = [first, second]
    assert list(bulk.pop_ready(closing)) == [] and closing == [first, second]    # the second's texts are there: it waits
    slow.set_result(({0: "text a"}, {}, 20, 0.25))
    assert list(bulk.pop_ready(closing)) == [first, second] and closing == []
    assert first.collect() == (20, 0.25) and first.texts == {0: "text a"} and first.retry == {}
    # at the end of the run the call blocks: batches leave in order whatever their futures say
    waiting = bulk.BatchRecord(["c"], 2, {}, [[0]])
    waiting.futures.append(Future())
    closing = [waiting, second]
    assert next(bulk.pop_ready(closing, block=True)) is waiting


def test_batch_record_collects_workers_results():
    paths = ["a", "b", "c", "d", "e"]
    batch = bulk.BatchRecord(paths, 0, {4: "e: truncated"}, [[0, 1], [2], [3]])
    batch.futures.append(_done(({0: "text a"}, {1: "b: track capacity exceeded"}, 30, 0.5)))
    batch.futures.append(_done(error=RuntimeError("worker died")))               # recording 2's group
    batch.futures.append(_done(({}, {}, 0, 0.25)))                               # answers for nobody: recording 3
    assert batch.unanswered() == [0, 1, 2, 3]                                    # nothing collected yet
    assert batch.collect() == (30, 0.75)
    assert batch.unanswered() == []
    assert batch.texts == {0: "text a"}
    assert batch.retry == {1: "b: track capacity exceeded", 2: "c: no metadata came back",
                           3: "d: no metadata came back", 4: "e: truncated"}
    # formatted in-process (no futures): a missing text is not the record's to explain
    plain = bulk.BatchRecord(paths, 0, {}, [[0, 1]])
    plain.texts[0] = "text a"
    assert plain.collect() == (0, 0.0) and plain.retry == {} and plain.unanswered() == [1]


def test_lane_rules():
    # waited > 0.2 x (lap + waited): the main thread sat waiting for the decode
    assert not bulk.decode_bound(waited=0.2, lap_s=0.8, decode_s=0.0)
    assert bulk.decode_bound(waited=0.21, lap_s=0.79, decode_s=0.0)
    # decode_s > 0.5 x lap: the decode's own duration against the first batch's turn
    assert not bulk.decode_bound(waited=0.0, lap_s=1.0, decode_s=0.5)
    assert bulk.decode_bound(waited=0.0, lap_s=1.0, decode_s=0.51)
    assert bulk.lane_share(1, 1024, 400000, 4 << 30) == (1024, 400000, 2048, 4 << 30)
    assert bulk.lane_share(2, 1024, 400000, 4 << 30) == (512, 200000, 1024, 2 << 30)
    share = bulk.lane_share(2, 100, 30000, 1001)
    assert (share.track_files, share.track_frames, share.cnn_chunk, share.network_bytes) == (64, 20000, 1024, 500)
    assert bulk.lane_share(1, 1, 100, 8)[:2] == (64, 20000)                      # the floors hold for one lane too
    assert bulk.lane_share(16, 1024, 400000, 1 << 20).cnn_chunk == 256
    gate = bulk.LaneGate(2)
    with gate.lane() as a:
        assert a in (0, 1) and gate.busy == 1
    assert gate.busy == 0 and sorted(gate.free) == [0, 1] and gate.limit == 1


def test_kept_tracks_order_and_region_rows():
    """Three clips of up to four tracks: clip 0 with a rejected track and two of equal rank, clip 1 failed, clip 2 with
    one track."""
    summ = np.zeros((3, 4), TRACK_SUMMARY_DTYPE)
    #                          reject rank start n_frames slot
    for b, j, row in ((0, 0, (0, 2, 3, 2, 1)), (0, 1, (5, 0, 0, 9, 0)), (0, 2, (0, 1, 1, 3, 2)), (0, 3, (0, 1, 4, 1, 0)),
                      (1, 0, (0, 0, 0, 5, 0)), (1, 1, (0, 1, 2, 4, 1)),
                      (2, 0, (0, 7, 2, 2, 3)), (2, 1, (0, 0, 0, 6, 0))):      # (clip 2 counts one track: row 1 is stale)
        for name, v in zip(("reject", "rank", "start_frame", "n_frames", "slot"), row):
            summ[b, j][name] = v
    ntr = np.array([4, 2, 1])
    counts = np.array([3, 2, 1])          # tracks the pipeline kept per clip: the failed clip keeps its two slots
    kept, kept_pipe = bulk.kept_tracks(summ, ntr, {1: "track capacity exceeded"}, counts)
    assert kept == [(0, 2), (0, 3), (0, 0), (2, 0)]       # ranks 1, 1 (in their order), 2; nothing of clip 1
    assert kept_pipe == [0, 1, 2, 5]                      # clip 2 starts at its prefix, 3 + 2
    offs = np.array([0, 10, 30, 40], np.int32)
    ma = 6
    rows, tr_off = bulk.kept_region_rows(summ, kept, offs, ma)
    assert tr_off.tolist() == [0, 3, 4, 6, 8] and tr_off.dtype == np.int64
    want = [(0 + 1 + q) * ma + 2 for q in range(3)] + [(0 + 4) * ma + 0] + [(0 + 3 + q) * ma + 1 for q in range(2)] \
        + [(30 + 2 + q) * ma + 3 for q in range(2)]
    assert rows.tolist() == want and rows.dtype == np.int64
    rows, tr_off = bulk.kept_region_rows(summ, [], offs, ma)
    assert len(rows) == 0 and tr_off.tolist() == [0]
    # the thumbnail requests: usable = not blank (flag 1) and with mass; the frame from the clip's processed-frame index
    regions = np.zeros(8, REGION_DTYPE)
    regions["mass"] = [5, 0, 7, 9, 1, 1, 3, 4]
    regions["flags"] = [0, 0, 1, 0, 0, 2, 0, 0]
    regions["frame_number"] = [1, 2, 3, 4, 3, 4, 0, 1]
    regions["x"], regions["width"] = np.arange(8), 10 + np.arange(8)
    proc_idx = [np.array([0, 2, 3, 5, 6, 7]), np.zeros(0, np.int64), np.array([31, 33])]
    usable, refs = bulk.usable_region_refs(regions, kept, np.asarray([0, 3, 4, 6, 8]), proc_idx)
    assert usable.tolist() == [0, 3, 4, 5, 6, 7]
    assert refs["frame"].tolist() == [2, 6, 5, 6, 31, 33]
    assert refs["x"].tolist() == [0, 3, 4, 5, 6, 7] and refs["width"].tolist() == [10, 13, 14, 15, 16, 17]
    usable, refs = bulk.usable_region_refs(np.zeros(0, REGION_DTYPE), [], np.zeros(1, np.int64), proc_idx)
    assert len(usable) == 0 and len(refs) == 0

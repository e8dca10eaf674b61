"""conv_block32s_kernel's halo carry (classifier-pipeline_amd/csrc/cpx_cnn_blk.hip): a tile whose right neighbour was the
workgroup's previous tile copies its mid columns 16 and 17 from that tile's buffer instead of computing them.  The same
float32 sums in the same order, so the logits are the SAME BITS as with CPX_BLOCK32_CARRY=0, on either walk
(CPX_BLOCK32_WALK: 1 = tile rows right to left, 0 = interleaved tiles, unset = the launcher's rule, which keeps the
interleaved tiles for batches this small) and on any grid.  The host build of the walk (tests/native/block_walk_host.cpp)
says how many tiles each launch carried, so that equality cannot pass with nothing carried."""
import numpy as np
import pytest
import torch

from test_block_walk_host import WALK_ROWS, build_host_lib, walk

pytestmark = pytest.mark.gpu

GRIDS = ("8", "24", None)  # CPX_BLOCK32_GRID; None = one workgroup per CU


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3")
    eng.set_cnn_math("fp16x2")
    yield eng
    eng.set_cnn_math(eng.DEFAULT_CNN_MATH)
    eng.close()


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return build_host_lib(tmp_path_factory.mktemp("block_walk_gpu") / "libblock_walk_host.so")


def _net(engine, side, n, seed):
    from cpx.ml_tools import wrresnet as wr

    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 255, size=(n, side, side, 2)).astype(np.float32)
    xd = torch.from_numpy(x).to(engine.device)
    w = wr.calibrate_bn_device(engine, wr.random_weights(17, seed=8), xd)
    return wr.WRResNetDevice(engine, w, 17), xd, w


def _forward(monkeypatch, net, xd, grid, walk_env, carry, taps=False):
    for name, value in (("CPX_BLOCK32_GRID", grid), ("CPX_BLOCK32_WALK", walk_env), ("CPX_BLOCK32_CARRY", carry)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    out = net.forward(xd, taps=True) if taps else net.forward(xd)
    for name in ("CPX_BLOCK32_GRID", "CPX_BLOCK32_WALK", "CPX_BLOCK32_CARRY"):
        monkeypatch.delenv(name, raising=False)
    return (out[0].clone(), out[3].copy()) if taps else out[0].clone()


def _grid_request(engine, grid):
    """What the launcher hands persistent_grid_x: CPX_BLOCK32_GRID, or the CUs shared among the two groups."""
    return int(grid) if grid else torch.cuda.get_device_properties(engine.device).multi_processor_count // 2


# stage-2 map side (= the input's): one tile; one carry per row; three tiles, the run starting on the ragged one (its
# carried columns are image columns 31 and 32); ragged 9 x 16 + 6; the bench's whole tiles
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("side", [16, 32, 37, 150, 160])
def test_carry_is_bitwise_the_computed_columns(engine, host_lib, monkeypatch, side, n):
    net, xd, _ = _net(engine, side, n, 300 + side)
    tiles = -(-side // 16)
    want = _forward(monkeypatch, net, xd, None, "0", "0")  # every tile computes its own columns, interleaved tiles
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0.0
    for grid in GRIDS:
        carried = walk(host_lib, tiles, tiles, n, _grid_request(engine, grid), WALK_ROWS)["carried"]
        assert carried == (tiles - 1) * tiles * n and (carried > 0 or side == 16), (grid, carried)
        on = _forward(monkeypatch, net, xd, grid, "1", None)
        off = _forward(monkeypatch, net, xd, grid, "1", "0")
        assert torch.equal(on, off), (grid, float((on - off).abs().max()))
        assert torch.equal(on, want), (grid, float((on - want).abs().max()))
        assert torch.equal(_forward(monkeypatch, net, xd, grid, None, None), want), grid  # the launcher's own choice
    assert not engine.cnn_last_overflow()
    net.close()


def test_overflow_in_a_carried_column_is_still_caught(engine, monkeypatch):
    """Two input pixels a million times the sensor's range, at map columns 15 and 32 (= 15 and 0 mod 16: the columns a
    left neighbour carries): the stage-2 blocks' activations around them leave fp16's range.  The carried pixels were
    range-checked by the tile that computed them, so with carry on and off alike the same blocks raise their overflow
    words, the forward says so, and the logits are the guarded three-plane reruns': bit for bit the same, and the exact
    mode's to float32 accuracy."""
    net, xd, w = _net(engine, 48, 2, 77)
    xd = xd.clone()
    xd[0, 20, 15, :] = 2.55e8
    xd[1, 30, 32, :] = 2.55e8
    from cpx.ml_tools import wrresnet as wr

    engine.set_cnn_math("bf16x3")
    exact_net = wr.WRResNetDevice(engine, w, 17)
    exact = exact_net.forward(xd)[0].clone()
    exact_net.close()
    engine.set_cnn_math("fp16x2")
    got = {}
    for carry in (None, "0"):
        logits, ovf = _forward(monkeypatch, net, xd, "8", "1", carry, taps=True)
        assert engine.cnn_last_overflow()
        assert ovf[1] or ovf[2], ovf  # (a block conv_block32s_kernel ran found it)
        assert torch.isfinite(logits).all()
        got[carry] = (logits, ovf)
    assert torch.equal(got[None][0], got["0"][0]) and np.array_equal(got[None][1], got["0"][1])
    tol = 2e-5 * max(1.0, float(exact.abs().max()))
    assert float((got[None][0] - exact).abs().max()) <= tol, (float((got[None][0] - exact).abs().max()), tol)
    net.close()

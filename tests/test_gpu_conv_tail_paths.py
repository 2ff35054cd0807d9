"""The paths of csrc/tg_conv.hip that the 18 cases of tests/test_gpu_conv_tail_abi.py never run, each through the same per-case body (grid bits,
derived bounds, dx_dev = NULL, a second backward byte-equal, guards): k_conv_fwd's four-channel-tile wave layout (Cout >= 128) with a partly
active second channel block, its short last chunk behind full ones, the linear forward's fall-back for bases that are not 16-byte aligned,
k_conv_bwd's last k block with its second tile inactive or partly valid, several partials over several channel blocks, k_conv_dx with a partly
valid second channel tile and with its packed table's fields at their tops (a 16 x 16 kernel, stride 4), k_conv_lin_dx with a partly valid k
tile over two batch tiles, the linear pair at stride 3, and the cap 2^25 / (Cout K) on the number of partials.  conv_tail_ref.route names the
path each case takes; tests/test_conv_tail_cpu.py checks that table without a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_tail_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conv_tail_device import _backward, _bits, _forward, check_case  # noqa: E402
from conv_tail_device import check_row_alone_equals_the_row_in_batches_of_65_and_33  # noqa: E402

f32 = np.float32

ALIGN_CASES = [(64, 3, 3, 64, 3, 3, 1, 5), (64, 1, 1, 32, 1, 1, 1, 33)]
OFFSETS = [(4, 0), (8, 0), (12, 0), (0, 4), (0, 8), (0, 12), (4, 4)]          # bytes past a 16-byte aligned address: (x, w)


@pytest.mark.parametrize("case", ref.PATH_CASES, ids=ref.case_id)
def test_grid_bits_random_bounds_repeat_and_null_dx(case):
    check_case(case)


@pytest.mark.parametrize("case", ALIGN_CASES, ids=ref.case_id)
def test_the_linear_forward_gives_the_same_bytes_at_every_alignment(case):
    """k_conv_lin_fwd reads 16-byte vectors; x or w at 4, 8 or 12 bytes past such an address takes k_conv_fwd.  Which kernel runs changes no bit."""
    stride = case[6]
    assert ref.route(case)["fwd"] == "lin" and ref.route(case, aligned=False)["fwd"] == "generic"
    rng = np.random.default_rng(13)
    x, w, b, _, _ = ref.grid_case(rng, case)
    want, _ = ref.forward(x, w, b, stride)
    aligned = _forward(x, w, b, stride)
    assert _bits(aligned, want.astype(f32))
    for xo, wo in OFFSETS:
        assert _bits(_forward(x, w, b, stride, x_offset=xo, w_offset=wo), aligned), (xo, wo)
    x, w, b, _, _ = ref.random_case(rng, case)
    aligned = _forward(x, w, b, stride)
    for xo, wo in OFFSETS:
        assert _bits(_forward(x, w, b, stride, x_offset=xo, w_offset=wo), aligned), (xo, wo)


@pytest.mark.parametrize("which", range(2), ids=["k80-o160", "k360"])
def test_forward_order_probes_give_zero_across_a_short_last_chunk(which):
    shape, triples = ref.path_forward_probe_sets()[which]
    x, w, b, at = ref.forward_probe(shape, triples)
    y = _forward(x, w, b, shape[6])
    got = np.array([y[i, i % shape[3], oy, ox] for i, (oy, ox) in enumerate(at)])
    assert _bits(got, np.zeros(len(at), f32)), [t for t, v in zip(triples, got) if v != 0][:8]       # any other order gives 1


@pytest.mark.parametrize("which", range(2), ids=["stride4", "kernel16"])
def test_dx_order_probes_give_zero_at_the_tops_of_the_table_fields(which):
    shape, at = ref.path_dx_probe_sets()[which]
    x, w, y, dy, B = ref.dx_probe(shape, at)
    _, _, dx = _backward(x, w, y, dy, shape[6])
    got = np.array([dx[i, i % shape[0], at[0], at[1]] for i in range(B)])
    assert _bits(got, np.zeros(B, f32)), [i for i, v in enumerate(got) if v != 0][:8]


@pytest.mark.parametrize("shape", [c[:7] for c in ref.PATH_CASES[:2]], ids=["o128", "o160"])
def test_a_row_alone_equals_the_row_in_batches_of_65_and_33(shape):
    assert ref.route(shape + (65,))["fwd_cl"] == 2
    check_row_alone_equals_the_row_in_batches_of_65_and_33(shape)


def test_the_cap_on_the_partials_binds():
    """(64, 16, 16, 512, 16, 16, 1, 1025): ceil(M / 256) = 5 but 2^25 / (Cout K) = 4, so P = 4 and the 17 chunks are walked 5, 4, 4, 4.  Grid
    inputs, no dx: dweight and dbias have the reference's bits.  About 0.3 GB on the device."""
    case = ref.CAP_CASE
    r = ref.route(case)
    assert r["cap_bound"] and r["P"] == 4 and -(-r["M"] // ref.BWD_SHARE) == 5
    assert [len(range(p, -(-r["M"] // ref.BWD_CHUNK), 4)) for p in range(4)] == [5, 4, 4, 4]
    x, w, b, y, dy = ref.grid_case(np.random.default_rng(17), case)
    dw, db, dx = _backward(x, w, y, dy, case[6], with_dx=False)
    assert dx is None
    want_dw, want_db = ref.dweight_dbias(x, w, y, dy, case[6])
    assert _bits(db, want_db.astype(f32))
    assert _bits(dw, want_dw.astype(f32))

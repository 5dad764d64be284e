"""The plain-torch restatements of tests/helpers_layout.py against torch itself, in float64 and without a GPU: the packed
operand layouts reproduce conv2d and its input gradient, the max-pool restatement reproduces max_pool2d and its autograd,
and the restated grid arithmetic shows which branches of the one-launch kernels the GPU cases of
test_step_helpers_gpu.py reach."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_layout as L

F64 = 1e-12       # float64 rounding only: sums of at most a few thousand products of O(1) numbers


def _pads(Ci, Co, R, S, eg=8):
    """operand extents as ConvOp lays them out (channels padded to the lane / 16, K padded to a 64-element stage)"""
    Ci_p, Co_p = -(-Ci // eg) * eg, -(-Co // 16) * 16
    rows_d = -(-Ci_p // 16) * 16
    kf_p = -(-(R * S * Ci_p) // 64) * 64
    kd_p = -(-(R * S * Co_p) // 64) * 64
    return Ci_p, Co_p, rows_d, kf_p, kd_p


CONVS = [  # Ci, Co, k, stride, pad, H, W, dgrad tap order
    (5, 6, 3, 1, 1, 7, 9, 0),
    (5, 6, 3, 2, 1, 8, 10, 1),
    (5, 6, 3, 2, 1, 7, 9, 1),       # odd extent: the class order is still a permutation of the same taps
    (11, 7, 1, 1, 0, 5, 6, 0),
    (11, 7, 1, 2, 0, 6, 8, 0),
    (3, 4, 7, 2, 3, 12, 14, 0),
]


@pytest.mark.parametrize("case", CONVS)
def test_packed_operands_reproduce_conv2d_and_its_input_gradient(case):
    Ci, Co, k, stride, pad, H, W, order = case
    g = torch.Generator().manual_seed(5 + Ci + k + stride)
    x = torch.randn(2, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    Ci_p, Co_p, rows_d, kf_p, kd_p = _pads(Ci, Co, k, k)

    w_f = L.packed_forward(w, Co_p, Ci_p, kf_p)
    got = torch.matmul(w_f, L.im2col_forward(x.detach(), k, k, stride, pad, Ci_p, kf_p))        # [N, Co_p, L]
    assert torch.equal(got[:, Co:], torch.zeros_like(got[:, Co:]))
    ref = y.detach().reshape(2, Co, -1)
    assert float((got[:, :Co] - ref).abs().max()) <= F64 * float(ref.abs().max())
    assert int((w_f != 0).sum()) == int((w != 0).sum())                      # nothing but the weights, each once

    w_d = L.packed_dgrad(w, rows_d, Co_p, kd_p, order)
    got = torch.matmul(w_d, L.im2col_dgrad(dy, H, W, k, k, stride, pad, Co_p, kd_p, order))     # [N, rows_d, H * W]
    assert torch.equal(got[:, Ci:], torch.zeros_like(got[:, Ci:]))
    ref = x.grad.reshape(2, Ci, -1)
    assert float((got[:, :Ci] - ref).abs().max()) <= F64 * float(ref.abs().max())
    assert int((w_d != 0).sum()) == int((w != 0).sum())
    if order == 1 and H % 2 == 0 and W % 2 == 0:
        # each parity class is a K slice of the operand: what the stride-2 data gradient kernels rely on
        got = L.dgrad_by_classes(w_d, dy, H, W, Ci, Co_p)
        assert float((got - x.grad).abs().max()) <= F64 * float(x.grad.abs().max())


def test_class_order_is_a_permutation_grouped_by_parity():
    assert sorted(L.S2_TAP_ORDER) == list(range(9))
    for (py, px), taps in L.S2_CLASSES.items():
        for pos, dr, ds in taps:
            r, s = divmod(L.S2_TAP_ORDER[pos], 3)
            # dx[2y'+py] reads dy[(2y'+py+1-r)/2]: r has the parity of py + 1 and the offset is (py + 1 - r) / 2
            assert (py + 1 - r) % 2 == 0 and (px + 1 - s) % 2 == 0
            assert (dr, ds) == ((py + 1 - r) // 2, (px + 1 - s) // 2)
    assert [pos for taps in L.S2_CLASSES.values() for pos, _, _ in taps] == list(range(9))
    assert L.tap_of(3, 1, 9) == 1 and L.tap_of(3, 0, 9) == 3 and L.tap_of(3, 1, 49) == 3


@pytest.mark.parametrize("shape", [(2, 3, 12, 20), (2, 3, 13, 21), (1, 2, 1, 1), (1, 2, 2, 3), (2, 3, 7, 1), (3, 2, 1, 9)])
def test_maxpool_restatement_equals_max_pool2d_and_autograd(shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(H * 31 + W)
    # tie-free: a permutation of distinct values, all negative (a zero pad would win every border window)
    x = (-1.0 - torch.randperm(N * C * H * W, generator=g).double()).view(N, C, H, W).requires_grad_(True)
    y_ref = F.max_pool2d(x, 3, 2, 1)
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    add = torch.randn(x.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)
    y, first = L.maxpool_ref(x.detach())
    assert torch.equal(y, y_ref.detach())
    assert torch.equal(first.sum(2), torch.ones_like(first.sum(2)))
    assert float((L.maxpool_grad_ref(first, dy, H, W) - x.grad).abs().max()) <= F64 * float(x.grad.abs().max())
    assert float((L.maxpool_grad_ref(first, dy, H, W, add) - (x.grad + add)).abs().max()) <= 4 * F64 * float((x.grad + add).abs().max())


def test_maxpool_restatement_takes_the_first_of_tied_maxima():
    x = torch.full((1, 1, 3, 3), -2.0, dtype=torch.float64)
    y, first = L.maxpool_ref(x)
    # windows (ho, wo) over the padded grid: the first in-range cell in row-major order wins each of them
    assert torch.equal(y, torch.full((1, 1, 2, 2), -2.0, dtype=torch.float64))
    assert first[0, 0, :, 0].nonzero().flatten().tolist() == [4]       # window (0,0): taps (1,1) is pixel (0,0)
    assert first[0, 0, :, 3].nonzero().flatten().tolist() == [0]       # window (1,1): tap (0,0) is pixel (1,1)
    dx = L.maxpool_grad_ref(first, torch.ones(1, 1, 2, 2, dtype=torch.float64), 3, 3)
    assert dx.flatten().tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0]


def test_upcat_pad_restatement_shapes_and_corners():
    a = torch.arange(2 * 4 * 1 * 3, dtype=torch.float64).view(2, 4, 1, 3).requires_grad_(True)
    b = torch.arange(2 * 4 * 2 * 6, dtype=torch.float64).view(2, 4, 2, 6)
    out = L.upcat_pad_ref(a, b)
    assert out.shape == (2, 8, 4, 8)
    assert torch.equal(out[:, :4, 0, 0], a[:, :, 0, 0]) and torch.equal(out[:, 4:, 3, 7], b[:, :, 1, 5])
    out.backward(torch.ones_like(out))
    # h = 1: a source pixel's two rows are the first and the last, so it gathers all 4 padded rows; an end pixel gathers
    # its 2 columns and the padded one (4 x 3 cells), the middle pixel its 2 columns (4 x 2)
    assert a.grad[0, 0].flatten().tolist() == [12.0, 8.0, 12.0]


# ---- which branches the GPU cases reach, from the restated host arithmetic ----
MiB = L.MiB
COPY_SIZES = L.COPY_SIZES


def test_copy_sizes_reach_every_branch_of_the_copy_kernel():
    gr = {n: L.copy_grid(n) for n in COPY_SIZES}
    assert gr[1]["n16"] == 0 and gr[15]["n16"] == 0 and gr[1]["tail"] == 1 and gr[15]["tail"] == 15       # tail only
    assert gr[16]["tail"] == 0 and gr[16]["n16"] == 1 and gr[17]["tail"] == 1                             # no tail / both
    assert gr[4101]["blocks"] == 1 and gr[4101]["rounds"] == {0} and gr[4101]["rest"] == {1} and gr[4101]["tail"] == 5
    assert gr[49159]["blocks"] == 3 and gr[49159]["rounds"] == {1} and gr[49159]["rest"] == {0}           # one unrolled round
    big = gr[8 * MiB + 16003]
    assert big["capped"] and big["blocks"] == 512 and big["rounds"] == {1} and big["rest"] == {0, 1} and big["tail"] == 3
    big = gr[24 * MiB + 9]
    assert big["capped"] and big["blocks"] == 512 and big["rounds"] == {3} and big["rest"] == {0} and big["tail"] == 9


CSUM_CASES = L.CSUM_CASES


def test_channel_sum_cases_reach_every_branch():
    gr = {c: L.csum_grid(*c) for c in CSUM_CASES}
    assert gr[(297, 16, 4)]["rounds"] == {0}                                  # the one shape the older unit test has
    assert {g["VL"] for g in gr.values()} == {4, 8}
    assert gr[(1100, 12, 2)]["VL"] == 4 and gr[(1100, 24, 2)]["VL"] == 8      # bf16: 8-byte and 16-byte lanes
    assert gr[(1100, 24, 2)]["CG"] == 3 and gr[(1100, 12, 2)]["CG"] == 3      # CG not a power of two: idle lanes in a block
    assert gr[(1, 12, 4)]["CG"] == 3
    for c in ((5000, 512, 4), (5000, 1024, 2), (8300, 512, 4)):
        assert gr[c]["gy"] == 2 and gr[c]["last_slab"] == 64 and gr[c]["gx"] == 256
    assert gr[(4100, 520, 2)]["gy"] == 2 and gr[(4100, 520, 2)]["last_slab"] == 1          # partly filled second slab
    assert set().union(*[g["rounds"] for g in gr.values()]) == {0, 1, 2}
    assert gr[(8300, 512, 4)]["rounds"] == {2} and gr[(1100, 16, 4)]["rounds"] == {0, 1}
    assert set().union(*[g["tails"] for g in gr.values()]) == {0, 1, 2, 3}
    # the multi form drops a bf16 batch with one C % 8 != 0 member to 4-channel lanes
    assert L.csum_grid(1100, 24, 2, wide=False)["VL"] == 4 and L.csum_grid(1100, 24, 2, wide=False)["CG"] == 6


PACK_LAYERS = L.PACK_LAYERS


def test_pack_layers_reach_every_tile_branch():
    br = {c: L.pack_tiles(c[1], c[0], c[2] * c[2]) for c in PACK_LAYERS}
    assert br[(64, 64, 3, 1, 1)] == {"3x3 full float4"}
    assert br[(40, 48, 3, 1, 1)] == {"3x3 full float4", "3x3 ragged"}
    assert br[(33, 32, 3, 1, 1)] == {"3x3 full scalar", "3x3 ragged"}        # Ci * 9 = 297 floats per row: not 16-byte multiples
    assert br[(16, 16, 3, 1, 1)] == {"3x3 ragged"} and br[(96, 32, 3, 1, 1)] == {"3x3 full float4"}
    assert br[(256, 64, 1, 1, 0)] == {"1x1 full"} and br[(192, 12, 1, 1, 0)] == {"1x1 ragged"}
    assert br[(64, 128, 1, 2, 0)] == {"1x1 ragged"}
    assert br[(3, 64, 7, 2, 3)] == {"generic"} and br[(6, 64, 7, 2, 3)] == {"generic"}

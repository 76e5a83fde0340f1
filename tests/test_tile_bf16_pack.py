"""CPU tests of the bf16 view of a generic pack (WRNN_ALGO_TILE_BF16, csrc/wrnn_tile_bf16.hip) through `wrnn_debug_tile_bf16_pack`, the packing routine
wrnn_pack_create runs on each of the eight loop matrices: the image holds exactly the round-to-nearest-even bfloat16 of every weight at the place the
kernel's lanes load it from, everything else is +0, a matrix with a value bfloat16 cannot hold is refused; and `synthetic.bf16_round_state_dict`, the
numpy restatement a user reproduces the kernel's model with, gives the same bits.  No HIP device is needed."""
import numpy as np
import pytest

TAIL_ROWS = 64
SHAPES = [(520, 19), (30, 257), (768, 525), (16, 8)]


def rne(W):
    """The rounding of the issue, restated: (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000 on the float32 bits."""
    u = np.ascontiguousarray(W, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)


def unpack(img, rows, K):
    """The image [ceil(K / 32) * rows + 64][4 kq][8 j] -> (the float32 bits of W[rows][K], a mask of the image elements that hold a weight)."""
    steps = -(-K // 32)
    assert img.dtype == np.uint16 and img.shape == (steps * rows + TAIL_ROWS, 4, 8)
    body = img[:steps * rows].reshape(steps, rows, 4, 8)
    k = np.arange(K)
    bits = body[k // 32, :, k % 4, (k % 32) // 4].T.astype(np.uint32) << 16         # [rows][K]
    used = np.zeros(img.shape, bool)
    used[:steps * rows].reshape(steps, rows, 4, 8)[k // 32, :, k % 4, (k % 32) // 4] = True
    return bits, used


@pytest.fixture(scope='module')
def pack():
    from wavernn_amd import _lib
    return _lib.tile_bf16_pack_host


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_the_image_holds_the_rne_rounding_of_every_weight_and_zeros_elsewhere(pack, shape):
    rows, K = shape
    rs = np.random.RandomState(rows * 1000 + K)
    W = (rs.standard_normal(shape) * np.exp(rs.uniform(-20, 20, shape))).astype(np.float32)
    W[rs.uniform(size=shape) < 0.05] = 0.0
    bits, used = unpack(pack(W), rows, K)
    assert np.array_equal(bits, rne(W))
    assert used.sum() == rows * K
    assert not pack(W)[~used].any()                 # K padding and the 64 rows behind the last k-step: +0, bit for bit
    assert (bits != W.view(np.uint32)).mean() > 0.9     # (the rounding did something)


def test_ties_signs_zeros_and_the_carry_into_the_next_binade(pack):
    cases = {
        0x3F808000: 0x3F800000,     # 1 + 2^-8: a tie, the even neighbour is below
        0x3F818000: 0x3F820000,     # 1 + 3 * 2^-8: a tie, the even neighbour is above
        0x3F808001: 0x3F810000,     # just above a tie: up
        0x3F807FFF: 0x3F800000,     # just below: down
        0xBF808000: 0xBF800000,     # the same ties, negative: the sign plays no part
        0xBF818000: 0xBF820000,
        0x3FFFFFFF: 0x40000000,     # 2 - 2^-23 rounds up into the next binade
        0x3FFF8000: 0x40000000,     # ... and so does the tie below it (odd neighbour below)
        0x00000000: 0x00000000,     # +0
        0x80000000: 0x80000000,     # -0 keeps its sign
        0x00000001: 0x00000000,     # the smallest denormal
        0x7F7F0000: 0x7F7F0000,     # the largest bfloat16
        0x7F7F7FFF: 0x7F7F0000,     # the largest float32 that still rounds to it
    }
    src = np.array(list(cases), np.uint32)
    W = np.zeros((16, 40), np.float32)
    W[3, 7:7 + len(src)] = src.view(np.float32)
    W[15, 39] = np.float32(-1.00390625)             # -(1 + 2^-8): the last element of the last row, in the K tail
    bits, used = unpack(pack(W), 16, 40)
    assert np.array_equal(bits, rne(W))
    assert [int(b) for b in bits[3, 7:7 + len(src)]] == list(cases.values())
    assert bits[15, 39] == 0xBF800000
    img = pack(W)
    assert (img[used.nonzero()] == 0x8000).sum() == 1 and not img[~used].any()       # one -0 among the weights, none in the padding


@pytest.mark.parametrize('bad', [0x7F7F8000, 0xFF7F8000, 0x7F800000, 0xFF800000, 0x7FC00000], ids=['rounds_to_inf', 'rounds_to_minus_inf', 'inf', 'minus_inf', 'nan'])
def test_a_value_bfloat16_cannot_hold_is_refused(pack, bad):
    from wavernn_amd import _lib
    W = np.ones((16, 8), np.float32)
    assert pack(W).shape == (16 + TAIL_ROWS, 4, 8)
    W[5, 3] = np.array([bad], np.uint32).view(np.float32)[0]
    with pytest.raises(_lib.WrnnError, match='rounds to'):
        pack(W)


def test_bf16_round_state_dict_gives_the_same_bits_and_leaves_the_rest_alone():
    import torch
    from wavernn_amd.synthetic import BF16_MATRICES, bf16_round_state_dict, random_state_dict
    sd = random_state_dict(5, mode='RAW', rnn_dims=72, fc_dims=40, bits=4, feat_dims=13, res_out_dims=20, compute_dims=8, res_blocks=1)
    before = {k: np.array(v, copy=True) for k, v in sd.items()}
    q = bf16_round_state_dict(sd)
    assert set(q) == set(sd) and len(BF16_MATRICES) == 8
    for k in sd:
        assert np.array_equal(np.asarray(sd[k]), before[k])                        # the input is not written to
        if k in BF16_MATRICES:
            assert q[k].dtype == np.float32 and np.array_equal(q[k].view(np.uint32), rne(before[k])) and not np.array_equal(q[k], before[k]), k
        else:                                                                       # biases, the up-sampling network, counters: the same objects
            assert q[k] is sd[k], k
    assert any(k.endswith('bias') for k in sd if k not in BF16_MATRICES) and any(k.startswith('upsample.') for k in sd)
    # idempotent, and torch tensors are taken too
    again = bf16_round_state_dict(q)
    assert all(np.array_equal(again[k], q[k]) for k in BF16_MATRICES)
    t = bf16_round_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    assert all(isinstance(t[k], torch.Tensor) and np.array_equal(t[k].numpy(), q[k]) for k in BF16_MATRICES)


def test_the_library_packs_what_bf16_round_state_dict_rounds(pack):
    from wavernn_amd.synthetic import bf16_round
    W = np.random.RandomState(3).uniform(-0.1, 0.1, (30, 257)).astype(np.float32)
    bits, _ = unpack(pack(W), 30, 257)
    assert np.array_equal(bits, bf16_round(W).view(np.uint32))
    assert np.array_equal(pack(bf16_round(W)), pack(W))

"""The weight permutation of the fused heads (vipe_conv2d_fused mode 7), on the host alone.

The kernel takes the B operand of its chained matrix instructions straight from the accumulators of the 128 -> 256
convolution: lane (pixel = lane % 16, k-group lk = lane / 16) of a 16 x 16 accumulator tile holds output channels
16 i + 4 lk + 0..3 of cout block i, and the blocks 2 ip and 2 ip + 1 side by side are the lane's 8 k-values.  This test
restates that layout on its own, multiplies it with the fragments `pack_heads2_fragments` builds - v_mfma_f32_16x16x32:
D[row, col] = sum over lk, e of A[lane = row + 16 lk][e] * B[lane = col + 16 lk][e] - and compares with the plain
256 -> 4 contraction per tap."""
import numpy as np
import torch


def _b_fragment(tile, s, h, ip):
    """[64 lanes, 8] values of the chained B operand for 16 pixels `tile` [16, 256] (fp16 values as float64)"""
    frag = np.zeros((64, 8))
    for lane in range(64):
        px, lk = lane % 16, lane // 16
        for e in range(8):
            i, r = 2 * ip + e // 4, e % 4          # accumulator tile (cout block) and register within it
            frag[lane, e] = tile[px, 128 * s + 64 * h + 16 * i + 4 * lk + r]
    return frag


def _mfma(a_frag, b_frag):
    d = np.zeros((16, 16))
    for row in range(16):
        for col in range(16):
            for lk in range(4):
                d[row, col] += a_frag[row + 16 * lk] @ b_frag[col + 16 * lk]
    return d


def test_fragment_product_equals_the_plain_contraction():
    from vipe_amd.slam.update_engine import heads2_fragment_index, pack_heads2_fragments
    g = torch.Generator().manual_seed(4)
    h2 = torch.zeros(4, 256, 3, 3, dtype=torch.float16)
    h2[0:2, 0:128] = (torch.randn(2, 128, 3, 3, generator=g) / 34.0).half()
    h2[2:4, 128:256] = (torch.randn(2, 128, 3, 3, generator=g) / 34.0).half()
    frags = pack_heads2_fragments(h2).double().numpy().reshape(2, 2, 2, 2, 64, 8)
    tile = torch.randn(16, 256, generator=g).relu().half().double().numpy()
    want = np.einsum("ockl,pc->klop", h2.double().numpy(), tile).reshape(9, 4, 16)  # [tap, out, pixel]
    for s in range(2):
        got = np.zeros((32, 16))
        for h in range(2):
            for rb in range(2):
                for ip in range(2):
                    got[16 * rb:16 * rb + 16] += _mfma(frags[s, h, rb, ip], _b_fragment(tile, s, h, ip))
        assert np.all(got[18:] == 0.0)                      # the padding rows of the 32-row A matrix
        rows = got[:18].reshape(9, 2, 16)                   # row = 2 tap + o
        assert np.abs(rows - want[:, 2 * s:2 * s + 2]).max() < 1e-12
    # every weight of the two diagonal blocks sits in exactly one valid fragment element
    out, ch, tap, valid = heads2_fragment_index()
    seen = np.zeros((4, 256, 9), dtype=np.int64)
    np.add.at(seen, (out[valid], ch[valid], tap[valid]), 1)
    block = np.zeros((4, 256, 9), dtype=bool)
    block[0:2, 0:128], block[2:4, 128:256] = True, True
    assert np.array_equal(seen, block.astype(np.int64))

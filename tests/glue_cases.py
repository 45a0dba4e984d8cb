"""Shapes and input draws shared by tests/test_glue_ref.py (CPU: the references and the reach of the bounds) and
tests/test_gpu_glue_kernels.py (the kernels) -- TEST ONLY.  Everything is float32 numpy drawn from a seeded generator."""
import numpy as np

# (taps, Cin, Cup) of lisec_head_compose / _backward.  kPairs = 16 (tap, c) pairs per workgroup, 16 n-slices, kMaxUp = 512:
#   (9, 8, 256)   72 pairs: the last workgroup has 8 dead pairs; the model's Cup
#   (4, 12, 40)   48 pairs, Cup not a multiple of 16 (n-slices of unequal length) and the ragged last 32-row block of
#                 k_head_compose_bwd_w (rows 32..39 live, 40..63 not)
#   (16, 4, 512)  Cup at the limit of the LDS copy of H
#   (1, 20, 17)   20 pairs: 12 dead in the second workgroup; Cup = 16 + 1: slice 0 alone has a second term
HEAD_CASES = [(9, 8, 256), (4, 12, 40), (16, 4, 512), (1, 20, 17)]


def head_inputs(taps, cin, cup, seed=0):
    """up_kernel (taps, Cup, Cin), up_bias (Cup,) with |bias| in [0.5, 1.5] (the bias_b[n] * S[j] term of d_head_w is as
    large as the rest), head_w (Cup, 16), G (taps, Cin, 16), S (16,), bias_in (16,)."""
    r = np.random.default_rng(1000 * seed + 100 * taps + 10 * cin + cup)
    f = np.float32
    return dict(up_kernel=(r.standard_normal((taps, cup, cin)) * 0.1).astype(f),
                up_bias=(r.choice([-1.0, 1.0], cup) * r.uniform(0.5, 1.5, cup)).astype(f),
                head_w=(r.standard_normal((cup, 16)) * 0.3).astype(f),
                G=r.standard_normal((taps, cin, 16)).astype(f),
                S=(r.standard_normal(16) * 4).astype(f),
                bias_in=r.standard_normal(16).astype(f))


# (ntaps, Cin, Cout) of lisec_const_field_grads:
#   (27, 64, 64)    the model's
#   (9, 12, 20)     ntaps * Cout = 180: k_const_field_gall's 256 threads are not all used, and nothing is a power of two
#   (27, 160, 128)  552 960 elements > 2048 workgroups x 256: the grid-stride loop of k_const_field_dw repeats
CONST_FIELD_CASES = [(27, 64, 64), (9, 12, 20), (27, 160, 128)]
CVEC_ROW_MAX = 3


def const_field_inputs(ntaps, cin, cout):
    """W (taps, Cin, Cout), S (taps, Cout), dW_old like W, table (CVEC_ROW_MAX + 2, Cin) whose LAST row is NaN: row
    CVEC_ROW_MAX + 1 exists, so an index that misses the clamp reads NaN instead of foreign memory."""
    r = np.random.default_rng(ntaps * 10007 + cin * 101 + cout)
    f = np.float32
    table = r.standard_normal((CVEC_ROW_MAX + 2, cin)).astype(f)
    table[-1] = np.nan
    return dict(W=(r.standard_normal((ntaps, cin, cout)) * 0.1).astype(f), S=(r.standard_normal((ntaps, cout)) * 5).astype(f),
                dW_old=r.standard_normal((ntaps, cin, cout)).astype(f), table=table)


# lisec_bn_finalize: 1024-thread workgroups of 16 columns x 64 row groups, loads batched 8 deep (b + 7*64 < nparts).
BN_C = [16, 24, 64, 256]                        # 24: half of the second workgroup's columns are dead
BN_NPARTS = [1, 63, 64, 65, 512, 513, 1030]     # 64 row groups: 63 / 64 / 65; the 8-deep batch: 512 / 513; two batches + tail
BN_ROWS = 2 * 1030 + 37


def bn_inputs(C, nparts, rows=BN_ROWS, negative_var_column=None):
    """A random (rows, C) fp32 map with |mean| <= 3 and std in [0.4, 2] per column (var >= 0.1 with margin: the fp64
    cancellation in s2/N - mean^2 loses at most a factor ~100 of 2^-53), cut into nparts ragged pieces whose
    (sum y, sum y^2) in fp64 are the partials; gamma, beta and starting moving statistics.
    negative_var_column: that column is one constant and its sums of squares are shaved by 1e-13 relative, so that
    s2/N - mean^2 comes out slightly NEGATIVE (what a differently ordered fp64 reduction can do to a constant channel)."""
    r = np.random.default_rng(C * 100003 + nparts * 17 + rows)
    y = (r.uniform(-3, 3, C) + r.uniform(0.4, 2.0, C) * r.standard_normal((rows, C))).astype(np.float32)
    if rows > 1:
        y -= (y.mean(0) - np.clip(y.mean(0), -3, 3)).astype(np.float32)
    if negative_var_column is not None:
        y[:, negative_var_column] = np.float32(2.7)
    cuts = np.sort(r.choice(np.arange(1, rows), nparts - 1, replace=False)) if nparts > 1 else np.zeros(0, int)
    pieces = np.split(y.astype(np.float64), cuts)
    partials = np.stack([np.stack([p.sum(0), (p * p).sum(0)]) for p in pieces])
    if negative_var_column is not None:
        partials[:, 1, negative_var_column] *= 1.0 - 1e-13
    f = np.float32
    return dict(y=y, partials=partials, gamma=r.uniform(0.5, 1.5, C).astype(f), beta=r.standard_normal(C).astype(f),
                moving_mean=r.uniform(-3, 3, C).astype(f), moving_var=r.uniform(0.5, 2.0, C).astype(f))


BN_FOLD_C = [16, 24, 100]                       # 100: not a multiple of the 64-thread workgroup


def bn_fold_inputs(C):
    """Moving variances log-spaced over 1e-6 .. 1e3 (shuffled), means in [-3, 3]."""
    r = np.random.default_rng(C)
    f = np.float32
    return dict(gamma=r.uniform(0.5, 1.5, C).astype(f), beta=r.standard_normal(C).astype(f),
                moving_mean=r.uniform(-3, 3, C).astype(f),
                moving_var=r.permutation(np.logspace(-6, 3, C)).astype(f))


# lisec_conv_tap_sums*: the two geometries of test_gpu_backward_ops.py's tap-sum test, and one whose Ho (5) is odd and
# smaller than the 16 line lanes of k_tap_sums (a lane's line index crosses more than one depth plane per step).
# (in_dims, out_dims, stride, pad, C), 3 x 3 x 3 taps
TAP_SUM_CASES = [((8, 16, 24), (4, 16, 24), (2, 1, 1), (1, 1, 1), 64),
                 ((4, 12, 40), (2, 12, 40), (1, 1, 1), (0, 1, 1), 64),
                 ((3, 5, 12), (2, 5, 12), (2, 1, 1), (1, 1, 1), 32)]

# (ntaps, K, N) of the weight packs: K and N padded to 64
PACK_CASES = [(27, 64, 64), (9, 80, 40), (1, 768, 16), (4, 20, 72)]


def bf16_edge_values():
    """fp32 values whose rounding to bf16 tells round-to-nearest-even from truncation, round-half-up and flushing:
    exact halves with an even and an odd kept mantissa (both signs), just above / below a half, signed zeros,
    subnormals (a half of the smallest bf16 subnormal, an odd half, the largest), and the largest finite float
    (rounds to infinity)."""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F817FFF, 0x00000000, 0x80000000,
            0x00000001, 0x00008000, 0x00018000, 0x80018000, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x3F7FFFFF]
    return np.array(bits, dtype=np.uint32).view(np.float32)

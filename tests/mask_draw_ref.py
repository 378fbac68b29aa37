"""CPU restatement of the device-side Mask-CTC mask draw (``tavsr_mask_uniform``, include/tavsr.h): Philox4x32-10 as csrc
keys it (csrc/common.h, csrc/dropout.hip) and ``mask_uniform_dev_ref``, the kernel's contract followed word for word.
The distribution is espnet's ``mask_uniform`` (n = randint(1, len + 1) positions drawn with replacement); the random stream
is the device generator's, so the GPU tests compare the kernel with this file bit for bit and the host tests check this
file's distribution."""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter: int, key: int):
    """the four 32-bit words of counter ``counter`` (64 bit, upper counter words 0) under key ``key`` (64 bit)"""
    c0, c1, c2, c3 = counter & M32, (counter >> 32) & M32, 0, 0
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        n0, n2 = (p1 >> 32) ^ c1 ^ k0, (p0 >> 32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def word(c: int, seed: int) -> int:
    """counter c -> word (c & 3) of philox(counter = c / 4): the element -> word mapping of tavsr_dropout"""
    return philox4x32_10(c >> 2, seed)[c & 3]


def mulhi(w: int, n: int) -> int:
    return (w * n) >> 32


def counters_per_row(Lmax: int) -> int:
    return (Lmax + 1 + 3) // 4 * 4


def mask_uniform_dev_ref(text, mask_token, eos, ignore_id, seed, offset, with_n=False):
    """text [B, Lmax] (array-like of ints) -> (ys_in, ys_out [B, Lmax] int64, n_target [B] int32) as numpy arrays;
    ``with_n``: a fourth result, the drawn n per row (0 for an empty row)"""
    text = np.asarray(text, dtype=np.int64)
    B, Lmax = text.shape
    seed &= 0xFFFFFFFFFFFFFFFF
    S = counters_per_row(Lmax)
    ys_in = np.full((B, Lmax), eos, dtype=np.int64)
    ys_out = np.full((B, Lmax), ignore_id, dtype=np.int64)
    n_target = np.zeros((B,), dtype=np.int32)
    ns = np.zeros((B,), dtype=np.int64)
    for b in range(B):
        toks = text[b][text[b] != ignore_id]
        ln = len(toks)
        ys_in[b, :ln] = toks
        if ln == 0:
            continue
        base = offset + b * S
        n = 1 + mulhi(word(base, seed), ln)
        ns[b] = n
        for j in range(n):
            idx = mulhi(word(base + 1 + j, seed), ln)
            ys_out[b, idx] = toks[idx]
            ys_in[b, idx] = mask_token
        n_target[b] = int((ys_out[b] != ignore_id).sum())
    return (ys_in, ys_out, n_target, ns) if with_n else (ys_in, ys_out, n_target)

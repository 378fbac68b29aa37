"""Copies, features and batch assembly: fills and strided copies, STFT / log-mel / SpecAugment, clip preparation, noise,
resampling, multi-tensor launches and the error-rate kernels.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import ops
from .._lib import check, lib, ptr, require_cuda, stream
from .base import _addr, empty, f32

__all__ = ["transpose_inner", "utterance_mvn", "fill_", "copy2d", "stft_frames", "power_spec", "log_mask", "time_warp", "specaug_mask_",
           "bucket_copy", "multi_add_", "multi_copy_", "video_prep", "add_noise", "resample", "edit_distance", "bootstrap_rates"]


def transpose_inner(x, nb, R, Cc, out=None):
    """out[n][c][r] = x[n][r][c] for a contiguous [nb, R, Cc] view of x."""
    require_cuda(x)
    if out is None:
        out = torch.empty_like(x)
    check(lib().tavsr_transpose_inner(ptr(x), ptr(out), nb, R, Cc, 0, stream()), "tavsr_transpose_inner")
    return out


def utterance_mvn(x, lens):
    B, T, F = x.shape
    require_cuda(x, lens)
    y = torch.empty_like(x)
    check(lib().tavsr_utterance_mvn(ptr(x), ptr(lens), ptr(y), B, T, F, stream()), "tavsr_utterance_mvn")
    return y


def fill_(t, value):
    require_cuda(t)
    assert t.is_contiguous()
    check(lib().tavsr_fill(ptr(t), value, t.numel(), stream()), "tavsr_fill")
    return t


def copy2d(src, dst):
    """dst[m, :N] = src[m, :N] for 2-D (row-strided) views of equal shape; no alignment requirement."""
    require_cuda(src, dst)
    assert src.shape == dst.shape and src.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
    check(lib().tavsr_copy2d(ptr(src), src.stride(0), ptr(dst), dst.stride(0), src.shape[0], src.shape[1], stream()), "tavsr_copy2d")
    return dst


# ---------------------------------------------------------------------------------------------- log-mel frontend, SpecAug
def stft_frames(wav, window, T, n_fft, hop, center=True):
    """wav [B, N] -> windowed frames [B*T, n_fft] (reflect padding of n_fft/2 when center)."""
    B, N = wav.shape
    require_cuda(wav, window)
    frames = empty(B * T, n_fft, like=wav)
    check(lib().tavsr_stft_frames(ptr(wav), ptr(window), ptr(frames), B, N, T, n_fft, hop, int(center), stream()), "tavsr_stft_frames")
    return frames


def power_spec(spec, nfreq, ldp, B, T, olens):
    """spec [B*T, >= 2*nfreq] (re | im) -> power [B*T, ldp] (zero K padding, zero past olens)."""
    require_cuda(spec, olens)
    P = empty(B * T, ldp, like=spec)
    check(lib().tavsr_power_spec(ptr(spec), spec.stride(0), ptr(P), ldp, nfreq, B, T, ptr(olens), stream()), "tavsr_power_spec")
    return P


def log_mask(mel, B, T, olens, floor=1e-10):
    require_cuda(mel, olens)
    out = torch.empty_like(mel)
    check(lib().tavsr_log_mask(ptr(mel), ptr(out), B, T, mel.shape[-1], ptr(olens), floor, stream()), "tavsr_log_mask")
    return out


def time_warp(x, center, warped, lens):
    """center / warped / lens: int64 [B] on the device (center 0 = leave that utterance unwarped)."""
    B, T, F = x.shape
    require_cuda(x, center, warped, lens)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    check(lib().tavsr_time_warp(ptr(x), ptr(y), B, T, F, ptr(center), ptr(warped), ptr(lens), stream()), "tavsr_time_warp")
    return y


def specaug_mask_(x, fpos=None, flen=None, tpos=None, tlen=None):
    """in place; band arrays [B, n] int64 on the device (None: that axis is not masked)."""
    B, T, F = x.shape
    require_cuda(x, fpos, flen, tpos, tlen)
    assert x.is_contiguous()
    nf = 0 if fpos is None else fpos.shape[1]
    nt = 0 if tpos is None else tpos.shape[1]
    check(lib().tavsr_specaug_mask(ptr(x), B, T, F, ptr(fpos), ptr(flen), nf, ptr(tpos), ptr(tlen), nt, stream()),
          "tavsr_specaug_mask")
    return x


def bucket_copy(ptrs, offs, sizes, n, flat, scale, to_flat, max_n):
    """pack (to_flat) or unpack-and-scale the tensors listed in the device tables into / from ``flat`` (tavsr/dp.py)."""
    require_cuda(ptrs, offs, sizes, flat)
    check(lib().tavsr_bucket_copy(ptr(ptrs), ptr(offs), ptr(sizes), int(n), ptr(flat), scale, int(bool(to_flat)), max_n, stream()),
          "tavsr_bucket_copy")


def multi_add_(dst, src):
    """dst[t] += src[t] for lists of contiguous fp32 tensors, one launch per 24 tensors."""
    assert len(dst) == len(src)
    if not dst:
        return dst
    require_cuda(*dst, *src)
    n = len(dst)
    for a, b in zip(dst, src):
        assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel() and a.dtype == f32 and b.dtype == f32
    dp = (C.c_void_p * n)(*[_addr(t) for t in dst])
    sp = (C.c_void_p * n)(*[_addr(t) for t in src])
    cnt = (C.c_int64 * n)(*[t.numel() for t in dst])
    check(lib().tavsr_multi_add(dp, sp, cnt, n, stream()), "tavsr_multi_add")
    return dst


def multi_copy_(dst, src, inc=None):
    """dst[t].copy_(src[t]) for lists of contiguous same-shape/dtype tensors in ONE launch (<= 24 tensors); ``inc`` (int64 tensor):
    every element incremented by one in the same launch."""
    assert len(dst) == len(src)
    require_cuda(*dst, *src)
    n = len(dst)
    for a, b in zip(dst, src):
        assert a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.numel() == b.numel()
    dp = (C.c_void_p * n)(*[_addr(t) for t in dst])
    sp = (C.c_void_p * n)(*[_addr(t) for t in src])
    cnt = (C.c_int64 * n)(*[t.numel() * t.element_size() for t in dst])
    if inc is not None:
        require_cuda(inc)
        assert inc.dtype == torch.int64 and inc.is_contiguous()
        check(lib().tavsr_multi_copy_inc(dp, sp, cnt, n, ptr(inc), inc.numel(), stream()), "tavsr_multi_copy_inc")
        return dst
    check(lib().tavsr_multi_copy(dp, sp, cnt, n, stream()), "tavsr_multi_copy")
    return dst


# ---------------------------------------------------------------------------------------------- batch assembly
def video_prep(src, index, T, y0, x0, th, tw, flip, affine, masked, out, pad_value):
    """one clip -> its row of the padded batch (tavsr_video_prep); ``index`` / ``masked`` are host lists / arrays or None."""
    require_cuda(src, out)
    dev = src.device
    Ts, H, W = src.shape
    frames = None if index is None else torch.tensor(index, dtype=torch.int32).to(dev)
    if frames is not None and T > 0 and (min(index) < 0 or max(index) >= Ts):
        raise ValueError("frame index outside the clip")
    m = None if masked is None or not masked.any() else torch.from_numpy(masked.astype("uint8")).to(dev)
    ws = empty(th * tw, like=out) if m is not None else None
    n = len(affine)
    mean = (C.c_float * 4)(*[a[0] for a in affine], *([0.0] * (4 - n)))
    std = (C.c_float * 4)(*[a[1] for a in affine], *([1.0] * (4 - n)))
    check(lib().tavsr_video_prep(ptr(src), int(src.dtype == torch.uint8), Ts, H, W, ptr(frames), int(T), int(y0), int(x0), int(th), int(tw),
                                 int(bool(flip)), mean, std, n, ptr(m), ptr(ws), ptr(out), int(out.shape[0]), pad_value, stream()),
          "tavsr_video_prep")
    return out


def add_noise(audio, noise, inv_snr):
    require_cuda(audio, noise)
    assert audio.numel() == noise.numel() and audio.is_contiguous() and noise.is_contiguous()
    out = torch.empty_like(audio)
    check(lib().tavsr_add_noise(ptr(audio), ptr(noise), ptr(out), audio.numel(), inv_snr, stream()), "tavsr_add_noise")
    return out


def resample(audio, factor: float):
    """band-limited resampling of a mono waveform [1, T] or [T] by ``factor`` (output length round(T / factor)): the clip played
    ``factor`` times faster at the same sample rate (tavsr_resample_sinc)"""
    require_cuda(audio)
    x = audio.float().contiguous().view(-1)
    n_out = lib().tavsr_resample_len(x.numel(), factor)
    y = empty(n_out, like=x)
    check(lib().tavsr_resample_sinc(ptr(x), x.numel(), ptr(y), n_out, factor, ops.RESAMPLE_ROLLOFF, ops.RESAMPLE_ZEROS, ops.RESAMPLE_BETA, stream()),
          "tavsr_resample_sinc")
    return y.view(*audio.shape[:-1], n_out)


# ---------------------------------------------------------------------------------------------- error rates
def edit_distance(ref, ref_off, hyp, hyp_off, n_pairs, max_len):
    """Levenshtein distance of n_pairs (reference, hypothesis) id sequences packed as (int32 ids, int64 offsets)."""
    require_cuda(ref, ref_off, hyp, hyp_off)
    assert ref.dtype == torch.int32 and hyp.dtype == torch.int32 and ref_off.dtype == torch.int64 and hyp_off.dtype == torch.int64
    assert ref_off.numel() == n_pairs + 1 and hyp_off.numel() == n_pairs + 1
    dist = torch.empty(n_pairs, dtype=torch.int32, device=ref.device)
    check(lib().tavsr_edit_distance(ptr(ref), ptr(ref_off), ptr(hyp), ptr(hyp_off), int(n_pairs), int(max_len), ptr(dist),
                                    stream()), "tavsr_edit_distance")
    return dist


def bootstrap_rates(dist, reflen, iters, seed):
    """100 * sum(dist[idx]) / sum(reflen[idx]) for ``iters`` resamples idx of the n sentences -> float64 [iters]."""
    require_cuda(dist, reflen)
    assert dist.dtype == torch.int32 and reflen.dtype == torch.int32 and dist.numel() == reflen.numel()
    rates = torch.empty(iters, dtype=torch.float64, device=dist.device)
    check(lib().tavsr_bootstrap_rates(ptr(dist), ptr(reflen), dist.numel(), int(iters), seed, ptr(rates), stream()),
          "tavsr_bootstrap_rates")
    return rates

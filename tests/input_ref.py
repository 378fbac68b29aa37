"""The kernels that turn raw data into model input, restated in plain torch / numpy: the log-mel frontend (framing, power, mel,
log), SpecAug (bicubic time warp, band masks), clip assembly (crop / mirror / re-index / Normalise chain / mean-frame masking /
padding), noise mixing and utterance mean normalisation.  The reference of tests/test_input_edges_host.py (which checks these
functions against oracle/leaves.py and oracle/data.py in float64) and of tests/test_gpu_input_edges.py (which checks
csrc/frontend.hip, csrc/data.hip and the utterance_mvn kernels of csrc/conv.hip against them).  The dtype follows the inputs:
called on ``.double()`` tensors it is the float64 reference, on fp32 tensors ``frames`` is the bit pattern the framing kernel must
produce (one fp32 multiply per value).  Nothing here imports the package under test.  Resampling has no restatement of its own:
``oracle.data.resample_sinc`` is numpy float64 already.

Reflect padding (no edge repeat): padded sample j of a length-N signal padded by p on both sides is x[reflect_index(j - p, N)]."""
import math

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ framing
def reflect_index(i, N):
    """source sample of position i in [-(N-1), 2(N-1)] of a reflect-padded length-N signal"""
    if i < 0:
        i = -i
    if i >= N:
        i = 2 * (N - 1) - i
    return i


def n_frames(N, n_fft, hop, center):
    return (N + (2 * (n_fft // 2) if center else 0) - n_fft) // hop + 1


def frames(wav, win, n_fft, hop, center):
    """wav [B, N], win [n_fft] -> [B, T, n_fft]: frame t holds win[n] * x_padded[t * hop + n], x_padded = wav reflect-padded by
    n_fft // 2 on both sides when ``center`` (the whole batch tensor is padded, not each utterance)"""
    if center:
        wav = F.pad(wav[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0, :]
    return wav.unfold(1, n_fft, hop) * win


# ------------------------------------------------------------------------------------------------ log-mel
def _hz_to_mel(f):
    f = torch.as_tensor(f, dtype=torch.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    return torch.where(f >= min_log_hz, min_log_hz / f_sp + torch.log(f.clamp(min=1e-10) / min_log_hz) / (math.log(6.4) / 27.0), f / f_sp)


def _mel_to_hz(m):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel = min_log_hz / f_sp
    return torch.where(m >= min_log_mel, min_log_hz * torch.exp(math.log(6.4) / 27.0 * (m - min_log_mel)), f_sp * m)


def mel_filterbank(fs, n_fft, n_mels, fmin=0.0, fmax=None):
    """Slaney-style triangular filters with area normalisation (librosa.filters.mel(htk=False, norm="slaney")): [n_mels, n_fft//2+1]
    float64"""
    fmax = fs / 2 if fmax is None else fmax
    freqs = torch.linspace(0, fs / 2, n_fft // 2 + 1, dtype=torch.float64)
    mel_f = _mel_to_hz(torch.linspace(float(_hz_to_mel(fmin)), float(_hz_to_mel(fmax)), n_mels + 2, dtype=torch.float64))
    fdiff = mel_f[1:] - mel_f[:-1]
    ramps = mel_f[:, None] - freqs[None, :]
    w = torch.clamp(torch.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]), min=0)
    return w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def hann_padded(win_length, n_fft):
    """periodic hann window of win_length samples centred in n_fft (torch.stft's padding of a short window), float64"""
    win = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    m = torch.arange(win_length, dtype=torch.float64)
    win[left:left + win_length] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * m / win_length)
    return win


def logmel(wav, lens, fs, n_fft, win_length, hop, center, n_mels, melmat=None):
    """wav [B, N] float64, lens [B] -> log-mel [B, T, n_mels] float64, olens [B].  ``melmat`` [n_fft//2+1, n_mels]: the filterbank
    to use instead of this module's float64 one (the host test passes the oracle's fp32-rounded one to compare at 1e-12)."""
    wav = wav.double()
    fr = frames(wav, hann_padded(win_length, n_fft), n_fft, hop, center)
    spec = torch.fft.rfft(fr, dim=-1)
    power = spec.real ** 2 + spec.imag ** 2                                   # [B, T, nfreq]
    olens = torch.div(lens.to(torch.int64) + (2 * (n_fft // 2) if center else 0) - n_fft, hop, rounding_mode="trunc") + 1
    dead = torch.arange(power.shape[1])[None, :] >= olens[:, None]            # [B, T]
    power = power.masked_fill(dead[:, :, None], 0.0)
    if melmat is None:
        melmat = mel_filterbank(fs, n_fft, n_mels).T
    mel = torch.log(torch.clamp(power @ melmat.double(), min=1e-10))
    return mel.masked_fill(dead[:, :, None], 0.0), olens


# ------------------------------------------------------------------------------------------------ SpecAug
def time_warp(x, center, warped, lens):
    """x [B, T, F]; per utterance b on its first lens[b] rows: rows [0, center) are resized to [0, warped) and rows [center, len) to
    [warped, len) by bicubic interpolation (align_corners=False, the frequency axis keeps its size); center == 0 copies the
    utterance; rows >= len are 0.  Rows >= len of the input are never read."""
    B, T, Fq = x.shape
    y = torch.zeros_like(x)
    for b in range(B):
        c, w, L = int(center[b]), int(warped[b]), int(lens[b])
        u = x[b, :L]
        if c == 0:
            y[b, :L] = u
            continue
        left = F.interpolate(u[None, None, :c], (w, Fq), mode="bicubic", align_corners=False)[0, 0]
        right = F.interpolate(u[None, None, c:], (L - w, Fq), mode="bicubic", align_corners=False)[0, 0]
        y[b, :L] = torch.cat([left, right], dim=0)
    return y


def band_hits(pos, length, D):
    """pos, length [B, n] -> bool [B, D]: d lies in one of the bands [pos, pos + length)"""
    ar = torch.arange(D)[None, None, :]
    return ((pos[:, :, None] <= ar) & (ar < (pos + length)[:, :, None])).any(dim=1)


def specaug_mask(x, fpos=None, flen=None, tpos=None, tlen=None):
    """x [B, T, F] with the frequency bands [fpos, fpos + flen) and the time bands [tpos, tpos + tlen) of each utterance set to 0
    (None: that axis is not masked); a new tensor"""
    B, T, Fq = x.shape
    hit = torch.zeros(B, T, Fq, dtype=torch.bool)
    if fpos is not None:
        hit = hit | band_hits(fpos, flen, Fq)[:, None, :]
    if tpos is not None:
        hit = hit | band_hits(tpos, tlen, T)[:, :, None]
    return x.masked_fill(hit, 0.0)


# ------------------------------------------------------------------------------------------------ clip assembly
def video_prep(src, index, T, y0, x0, th, tw, flip, affine, masked, Tpad, pad):
    """src [Ts, H, W] (uint8 or float) -> float64 [Tpad, th, tw]: output frame t < T is source frame index[t] (t when index is None),
    cropped to rows [y0, y0 + th) and columns [x0, x0 + tw), mirrored left-right when ``flip``, then put through (v - mean) / std for
    every (mean, std) of ``affine`` in order; frames with masked[t] are replaced by the mean over the T frames so prepared; frames
    t >= T hold ``pad``"""
    out = torch.full((Tpad, th, tw), float(pad), dtype=torch.float64)
    if T == 0:
        return out
    sel = torch.arange(T) if index is None else torch.as_tensor(list(index[:T]), dtype=torch.int64)
    v = src[sel].double()[:, y0:y0 + th, x0:x0 + tw]
    if flip:
        v = v.flip(-1)
    for mean, std in affine:
        v = (v - mean) / std
    if masked is not None:
        m = torch.as_tensor(masked, dtype=torch.bool)
        if bool(m.any()):
            v = torch.where(m[:, None, None], v.mean(0, keepdim=True), v)
    out[:T] = v
    return out


def add_noise(audio, noise, inv_snr):
    """audio + inv_snr * noise * sqrt(P_audio / P_noise), P = mean of squares"""
    pa, pn = (audio ** 2).sum() / audio.numel(), (noise ** 2).sum() / noise.numel()
    return audio + inv_snr * noise * torch.sqrt(pa / pn)


def utterance_mvn(x, lens):
    """x [B, T, F]: every utterance minus the mean of its first lens[b] rows; rows >= lens[b] are 0"""
    B, T, _ = x.shape
    live = (torch.arange(T)[None, :] < lens[:, None])[:, :, None]
    xm = x.masked_fill(~live, 0.0)
    mean = xm.sum(1, keepdim=True) / lens.to(x.dtype)[:, None, None]
    return (xm - mean).masked_fill(~live, 0.0)

"""The kernels that turn raw data into model input (csrc/frontend.hip: stft_frames, power_spec, log_mask, time_warp, specaug_mask;
csrc/data.hip: video_prep with video_mean_frame, add_noise, resample_sinc; the utterance_mvn kernels of csrc/conv.hip) through
``tavsr.ops``, each against the float64 restatements of tests/input_ref.py (validated on the host by tests/test_input_edges_host.py)
or the oracle's numpy resampling, at the geometries where their index logic takes another path:

a. framing, bit for bit: N = pad + 1, n_fft below / at / above the 256-thread loop, no centring, one frame; the two refusals.
b. power with a padded spectrum row, NaN in everything the kernel must not use, frame counts 0, T and beyond T.
c. log + length mask on the clamp's edge values.
d. the whole DefaultFrontend at four geometries on signals whose spectrum is not flat (tone, DC, burst then silence, quiet):
   kernel error <= max(2e-4, 4 e32), e32 = the error of the oracle's fp32 frontend (torch.stft) on the host against the same float64
   reference; 2e-4 is the bar of tests/test_gpu_frontend.py, 4 the project's margin for another summation order.
e. time warp at every (center, warped) pair espnet2 can draw for 16 frames and a window of 4, and on a ragged batch whose rows past
   each utterance are NaN: bound max(1e-5 max|x|, 4 e32), e32 = F.interpolate in fp32 on the host.
f. SpecAug masks with explicit bands (length 0, position 0, ending at the axis' size, reaching past it, overlapping), exact.
g. noise mixing at lengths around the 1024-thread loop, h. resampling down to one sample, i. clip assembly called directly (every
   corner window, mirror, 0..4 Normalise steps, re-indexing, mean-frame masks, padding, a 1000-frame mean), j. utterance mean
   normalisation of a near-constant utterance (mean / spread = 2300) on the vector (F = 80) and the scalar (F = 81) kernel: bound
   max(1e-5 max|ref|, 4 e32), e32 = ``x - x.sum(0) / T`` in fp32 on the device.

Sections d, e and j print every figure (profiles/input_edges.txt)."""
import math

import numpy as np
import pytest
import torch

import input_ref as R
from oracle import leaves as L
from oracle.data import resample_sinc

pytestmark = pytest.mark.gpu

FS = 16000


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _i64(v):
    return torch.as_tensor(v, dtype=torch.int64).cuda()


# ------------------------------------------------------------------------------------------------ a. stft_frames
FRAME_GEOMETRIES = [(512, 160, True, 257, 1), (512, 160, True, 4123, 3), (400, 160, True, 1000, 2), (30, 7, False, 100, 2),
                    (600, 200, True, 1000, 1), (512, 160, False, 512, 1)]


@pytest.mark.parametrize("n_fft,hop,center,N,B", FRAME_GEOMETRIES)
def test_stft_frames_bit_for_bit(n_fft, hop, center, N, B):
    """each frame value is one fp32 multiply of a window value and the sample the reflect index map names"""
    from tavsr import ops
    g = _gen(n_fft + N)
    wav = torch.arange(B * N, dtype=torch.float32).view(B, N) / 64 + torch.randn(B, N, generator=g)      # distinct values: a wrong index shows
    win = torch.rand(n_fft, generator=g) + 0.25                                                          # no symmetry, no zeros
    T = R.n_frames(N, n_fft, hop, center)
    want = R.frames(wav, win, n_fft, hop, center)
    assert want.dtype == torch.float32 and want.shape == (B, T, n_fft)
    got = ops.stft_frames(wav.cuda(), win.cuda(), T, n_fft, hop, center)
    assert got.shape == (B * T, n_fft) and torch.equal(got.cpu().view(B, T, n_fft), want)


def test_stft_frames_refuses_what_does_not_fit():
    from tavsr import ops
    from tavsr._lib import TavsrError
    win = torch.ones(512).cuda()
    with pytest.raises(TavsrError, match="reflect padding"):
        ops.stft_frames(torch.zeros(1, 256).cuda(), win, 1, 512, 160, True)                # N == pad: torch refuses it as well
    wav = torch.zeros(2, 1000).cuda()
    T = R.n_frames(1000, 512, 160, True)
    ops.stft_frames(wav, win, T, 512, 160, True)
    with pytest.raises(TavsrError, match="do not fit"):
        ops.stft_frames(wav, win, T + 1, 512, 160, True)
    with pytest.raises(TavsrError, match="do not fit"):
        ops.stft_frames(wav, win, R.n_frames(1000, 512, 160, False) + 1, 512, 160, False)


# ------------------------------------------------------------------------------------------------ b. power_spec
@pytest.mark.parametrize("nfreq,ldp", [(257, 288), (16, 32)])
def test_power_spec_uses_only_live_rows_and_columns(nfreq, ldp):
    from tavsr import ops
    B, T, ld = 4, 5, 2 * nfreq + 6
    olens = torch.tensor([0, T, T + 3, 2])
    g = _gen(nfreq)
    buf = torch.randn(B * T, ld, generator=g) * 3
    buf[:, 2 * nfreq:] = float("nan")
    live = (torch.arange(T)[None, :] < olens[:, None]).reshape(-1)                         # [B*T]
    buf[~live] = float("nan")
    spec = buf.cuda()[:, :2 * nfreq]
    assert spec.stride(0) == ld > 2 * nfreq
    P = ops.power_spec(spec, nfreq, ldp, B, T, olens.cuda()).cpu()
    assert P.shape == (B * T, ldp)
    re, im = buf[live, :nfreq].double(), buf[live, nfreq:2 * nfreq].double()
    want = re ** 2 + im ** 2
    assert bool(((P[live, :nfreq].double() - want).abs() <= 1e-6 * want).all())
    assert bool((P[live, nfreq:] == 0).all()) and bool((P[~live] == 0).all())
    assert int(live.sum()) == T + T + 2


# ------------------------------------------------------------------------------------------------ c. log_mask
@pytest.mark.parametrize("B,T,n_mels", [(3, 11, 9), (2, 3, 7)])
def test_log_mask_on_the_clamp_edges(B, T, n_mels):
    from tavsr import ops
    n = B * T * n_mels
    assert n % 256 != 0
    mel = torch.rand(B, T, n_mels, generator=_gen(n)) * 98 + 2
    mel[:, :, :7] = torch.tensor([0.0, 1e-12, 1e-10, -1.0, 1e-30, 1.0, 1e30])                 # in every row
    olens = torch.tensor([T, T // 3, 0][:B])
    live = torch.arange(T)[None, :] < olens[:, None]
    mel[~live] = float("nan")
    out = ops.log_mask(mel.cuda(), B, T, olens.cuda()).cpu()
    want = torch.log(torch.clamp(mel[live].double(), min=1e-10))
    assert bool(((out[live].double() - want).abs() <= 1e-6 * want.abs()).all())
    assert bool((out[~live] == 0).all())
    assert bool((out[live][mel[live] == 1.0] == 0).all()) and float(out[live].min()) < -23.0 and float(out[live].max()) > 69.0


# ------------------------------------------------------------------------------------------------ d. frontend end to end
N_SAMPLES, LENS = 4000, [4000, 3001, 1700]


def _signal(kind, g):
    t = torch.arange(N_SAMPLES, dtype=torch.float64)[None, :]
    if kind == "uniform":
        x = 0.1 * (2 * torch.rand(3, N_SAMPLES, generator=g, dtype=torch.float64) - 1)
    elif kind == "tone+noise":
        x = 0.5 * torch.sin(2 * math.pi * 1000 * t / FS) + 1e-4 * torch.randn(3, N_SAMPLES, generator=g, dtype=torch.float64)
    elif kind == "dc+noise":
        x = 0.5 + 1e-3 * torch.randn(3, N_SAMPLES, generator=g, dtype=torch.float64)
    elif kind == "burst/silence":
        x = 0.5 * torch.randn(3, N_SAMPLES, generator=g, dtype=torch.float64)
        x[:, 2000:] = 0.0
    else:
        assert kind == "quiet", kind
        x = 1e-4 * torch.randn(3, N_SAMPLES, generator=g, dtype=torch.float64)
    return x.float()                     # the fp32 waveform every implementation gets; the reference takes it as float64


GEOMETRIES = [(512, 400, 160, True, 80), (400, 400, 160, True, 80), (64, 48, 20, True, 20), (30, 30, 7, False, 20)]
FRONTEND_CASES = ([(GEOMETRIES[0], k) for k in ("uniform", "tone+noise", "dc+noise", "burst/silence", "quiet")]
                  + [(geo, k) for geo in GEOMETRIES[1:] for k in ("uniform", "tone+noise")])


@pytest.mark.parametrize("geo,kind", FRONTEND_CASES, ids=lambda v: v.replace("/", "_") if isinstance(v, str) else "x".join(map(str, v)))
def test_frontend_on_signals_that_are_not_flat(geo, kind):
    from tavsr.frontend.default import DefaultFrontend
    n_fft, win, hop, center, n_mels = geo
    wav, lens = _signal(kind, _gen(n_fft + len(kind))), torch.tensor(LENS)
    want, olens_want = R.logmel(wav.double(), lens, FS, n_fft, win, hop, center, n_mels)
    kw = dict(fs=FS, n_fft=n_fft, win_length=win, hop_length=hop, center=center, n_mels=n_mels)
    f32, olens32 = L.DefaultFrontend(**kw)(wav, lens)
    got, olens = DefaultFrontend(**kw)(wav.cuda(), lens.cuda())
    got = got.cpu()
    assert olens.cpu().tolist() == olens_want.tolist() == olens32.tolist()
    assert got.shape == want.shape
    live = (torch.arange(want.shape[1])[None, :] < olens_want[:, None])[:, :, None].expand_as(want)
    assert bool((got[~live] == 0).all()) and int((~live).sum()) > 0
    loud = live & (want >= want.max(-1, keepdim=True).values - math.log(1e6))          # within 60 dB of the frame's largest mel power
    ek, e32 = (got.double() - want).abs(), (f32.double() - want).abs()
    bound = max(2e-4, 4 * float(e32[live].max()))
    ok = float(ek[live].max()) <= bound
    tag = f"frontend {'x'.join(map(str, geo)):<22s} {kind:<13s}"
    for name, sel in (("all live bins", live), ("within 60 dB ", loud)):
        k, e = float(ek[sel].max()), float(e32[sel].max())
        print(f"{tag} {name} kernel {k:.2e}  e32 {e:.2e}  ratio {k / max(e, 1e-30):7.2f}  bound {bound:.1e}  {'ok' if k <= bound else 'FAIL'}")
    b, t, m = np.unravel_index(int(torch.where(live, ek, -torch.ones_like(ek)).argmax()), ek.shape)
    print(f"{tag} worst bin     utterance {b} frame {t} mel {m}: reference {float(want[b, t, m]):.4f}, frame maximum {float(want[b, t].max()):.4f}")
    assert ok, (float(ek[live].max()), bound)


# ------------------------------------------------------------------------------------------------ e. time_warp
def _warp_check(tag, x, center, warped, lens):
    """x fp32 on the host (rows past an utterance may be NaN) -> the kernel's output; asserts section e's bound on the live rows"""
    from tavsr import ops
    want = R.time_warp(x.double(), center, warped, lens)
    h32 = R.time_warp(x, center, warped, lens)
    got = ops.time_warp(x.cuda(), _i64(center), _i64(warped), _i64(lens)).cpu()
    live = (torch.arange(x.shape[1])[None, :] < torch.as_tensor(lens)[:, None])[:, :, None].expand_as(x)
    assert bool(torch.isfinite(got).all()) and bool((got[~live] == 0).all())
    ek, e32 = float((got.double() - want)[live].abs().max()), float((h32.double() - want)[live].abs().max())
    bound = max(1e-5 * float(x[live].abs().max()), 4 * e32)
    print(f"warp {tag:<28s} kernel {ek:.2e}  e32 {e32:.2e}  ratio {ek / max(e32, 1e-30):7.2f}  bound {bound:.1e}  {'ok' if ek <= bound else 'FAIL'}")
    assert ek <= bound, (ek, bound)
    return got


def test_time_warp_at_every_pair_espnet_can_draw():
    """L = 16, window 4: center in [4, 12), warped in [center - 3, center + 4] - 64 pairs, one per batch row; warped = 1 (a one-row
    left segment) and warped = 15 (a one-row right segment) are among them"""
    pairs = [(c, w) for c in range(4, 12) for w in range(c - 3, c + 5)]
    assert len(pairs) == 64 and (4, 1) in pairs and (11, 15) in pairs
    x = torch.randn(64, 16, 3, generator=_gen(16))
    _warp_check("64 pairs T=16 F=3", x, [p[0] for p in pairs], [p[1] for p in pairs], [16] * 64)


@pytest.mark.parametrize("Fq", [80, 1])
def test_time_warp_of_a_ragged_batch_never_reads_past_an_utterance(Fq):
    lens, center, warped = [16, 11, 8, 16], [4, 6, 0, 11], [1, 10, 0, 15]
    x = torch.randn(4, 18, Fq, generator=_gen(Fq))
    for b, le in enumerate(lens):
        x[b, le:] = float("nan")
    got = _warp_check(f"ragged T=18 F={Fq}", x, center, warped, lens)
    assert torch.equal(got[2, :8], x[2, :8])                                  # center = 0: the utterance is copied


# ------------------------------------------------------------------------------------------------ f. specaug_mask_
def _bands(B, D):
    """[B, 3] positions and lengths on an axis of size D: length 0 at position 0, a band ending exactly at D, two overlapping bands,
    one reaching past the axis, one starting at D"""
    pos = torch.tensor([[0, D - 2, 1], [D - 1, 1, 2], [0, D, 3]])[:B]
    length = torch.tensor([[0, 2, 3], [5, 3, 3], [2, 1, 0]])[:B]
    return pos, length


@pytest.mark.parametrize("B,T,Fq", [(3, 9, 7), (2, 50, 13)])
@pytest.mark.parametrize("axes", ["freq", "time", "both", "neither"])
def test_specaug_mask_with_explicit_bands(B, T, Fq, axes):
    from tavsr import ops
    x = torch.randn(B, T, Fq, generator=_gen(T)) + 4
    fpos = flen = tpos = tlen = None
    if axes in ("freq", "both"):
        fpos, flen = _bands(B, Fq)
        x[0, :, Fq - 1] = float("nan")                                          # under the band that ends exactly at F
    if axes in ("time", "both"):
        tpos, tlen = _bands(B, T)
        x[0, T - 1, :] = float("nan")
        x[1, 1, 0] = float("nan")                                               # under the first of the overlapping bands
    want = R.specaug_mask(x, fpos, flen, tpos, tlen)
    assert not bool(torch.isnan(want).any())
    xd = x.cuda()
    y = ops.specaug_mask_(xd, *(None if t is None else t.cuda() for t in (fpos, flen, tpos, tlen)))
    assert y is xd and torch.equal(y.cpu(), want)
    if axes == "neither":
        assert torch.equal(y.cpu(), x)
    else:
        assert 0 < int((want == 0).sum()) < want.numel()


# ------------------------------------------------------------------------------------------------ g. add_noise
@pytest.mark.parametrize("n", [1, 7, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("inv_snr", [0.1, 3.0])
def test_add_noise_around_the_block_size(n, inv_snr):
    from helpers import max_rel
    from tavsr import ops
    g = _gen(n)
    audio, noise = 1e-3 * torch.randn(1, n, generator=g) + 0.2, 100 * torch.randn(1, n, generator=g)
    out = ops.add_noise(audio.cuda(), noise.cuda(), inv_snr)
    assert out.shape == audio.shape
    assert max_rel(out.cpu(), R.add_noise(audio.double(), noise.double(), inv_snr)) <= 1e-6


# ------------------------------------------------------------------------------------------------ h. resample
@pytest.mark.parametrize("n_in", [1, 5, 300, 1000])
@pytest.mark.parametrize("factor", [0.5, 0.9, 1.1, 2.0])
def test_resample_of_short_clips(n_in, factor):
    from tavsr import ops
    x = torch.randn(1, n_in, generator=_gen(n_in))
    ref = resample_sinc(x.numpy(), factor)
    assert len(ref) == int(round(n_in / factor))
    y = ops.resample(x.cuda(), factor)
    assert y.shape == (1, len(ref))
    if len(ref):
        assert np.abs(y.cpu().numpy().reshape(-1).astype(np.float64) - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


# ------------------------------------------------------------------------------------------------ i. video_prep
AFFINE = [(0.0, 250.0), (0.421, 0.165), (0.1, 2.0), (-0.2, 1.5)]
PAD = -1.0


def _clip(dtype, Ts, H, W, seed):
    g = _gen(seed)
    raw = torch.randint(0, 256, (Ts, H, W), generator=g, dtype=torch.uint8)
    return raw if dtype == torch.uint8 else raw.float() + torch.rand(Ts, H, W, generator=g)


def _prep_check(src, src_d, index, T, y0, x0, th, tw, flip, affine, masked, Tpad):
    from tavsr import ops
    tag = (index, T, y0, x0, th, tw, flip, len(affine), None if masked is None else masked.nonzero()[0].tolist(), Tpad)
    out = torch.full((Tpad, th, tw), 7.0, device="cuda")
    assert ops.video_prep(src_d, index, T, y0, x0, th, tw, flip, affine, masked, out, PAD) is out
    want = R.video_prep(src, index, T, y0, x0, th, tw, flip, affine, masked, Tpad, PAD)
    out = out.cpu()
    err = float((out[:T].double() - want[:T]).abs().max()) if T else 0.0
    assert err <= 2e-6, (tag, err)
    assert bool((out[T:] == PAD).all()), tag                                     # pad frames are exact
    if not affine and (masked is None or not masked.any()):
        assert torch.equal(out[:T].double(), want[:T]), tag                       # a pure gather
    return err


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_video_prep_windows_mirror_and_normalise_chains(dtype):
    """[9, 11, 13] clip: the 5 x 7 window in each corner (y0 + th == H, x0 + tw == W among them) and the whole frame, mirrored or
    not, through 0, 1, 2 and 4 Normalise steps"""
    Ts, H, W = 9, 11, 13
    src = _clip(dtype, Ts, H, W, 1)
    src_d = src.cuda()
    windows = [(y0, x0, 5, 7) for y0 in (0, H - 5) for x0 in (0, W - 7)] + [(0, 0, H, W)]
    worst = 0.0
    for y0, x0, th, tw in windows:
        for flip in (False, True):
            for n_aff in (0, 1, 2, 4):
                worst = max(worst, _prep_check(src, src_d, None, Ts, y0, x0, th, tw, flip, AFFINE[:n_aff], None, Ts))
    print(f"video_prep windows {dtype}: worst error {worst:.2e}")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_video_prep_reindexing_masks_and_padding(dtype):
    Ts, H, W = 9, 11, 13
    src = _clip(dtype, Ts, H, W, 2)
    src_d = src.cuda()
    worst = 0.0
    for index in (None, list(range(Ts - 1, -1, -1)), [0, 0, 3, 8, 8, 2, 2]):
        T = Ts if index is None else len(index)
        masks = [None, np.zeros(T, dtype=bool)]
        for on in ([0], [T - 1], list(range(T))):
            m = np.zeros(T, dtype=bool)
            m[on] = True
            masks.append(m)
        for masked in masks:
            for Tpad in (T, T + 3):
                for flip in (False, True):
                    worst = max(worst, _prep_check(src, src_d, index, T, H - 5, W - 7, 5, 7, flip, AFFINE[:2], masked, Tpad))
    _prep_check(src, src_d, None, 0, 0, 0, 5, 7, False, AFFINE[:2], None, 3)                          # T = 0: padding only
    _prep_check(src, src_d, [], 0, 0, 0, 5, 7, True, AFFINE[:2], np.zeros(0, dtype=bool), 3)
    print(f"video_prep index / mask / pad {dtype}: worst error {worst:.2e}")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_video_prep_window_of_more_than_one_block(dtype):
    """17 x 19 = 323 pixels of a 20 x 20 clip: the mean frame takes two blocks, the window ends at the frame's last row and column"""
    src = _clip(dtype, 4, 20, 20, 3)
    masked = np.array([False, True, False, True])
    for flip in (False, True):
        _prep_check(src, src.cuda(), [3, 1, 1, 0], 4, 3, 1, 17, 19, flip, AFFINE[:2], masked, 5)


def test_video_prep_mean_frame_of_a_long_clip():
    """T = 1000: the mean frame is a sequential fp32 sum of 1000 values of size ~0.65, under the same 2e-6"""
    T = 1000
    src = _clip(torch.uint8, T, 11, 13, 4)
    masked = np.zeros(T, dtype=bool)
    masked[::10] = True
    err = _prep_check(src, src.cuda(), None, T, 3, 2, 5, 7, True, AFFINE[:2], masked, T)
    mean = R.video_prep(src, None, T, 3, 2, 5, 7, True, AFFINE[:2], masked, T, PAD)[0]
    print(f"video_prep T=1000 mean frame: error {err:.2e} at |mean| <= {float(mean.abs().max()):.2f}")


def test_video_prep_refuses_windows_and_frames_outside_the_clip():
    from tavsr import ops
    from tavsr._lib import TavsrError
    src = _clip(torch.uint8, 9, 11, 13, 5).cuda()
    out = torch.empty(9, 5, 7, device="cuda")
    for y0, x0 in ((7, 0), (0, 7), (-1, 0), (0, -1)):
        with pytest.raises(TavsrError, match="crop window"):
            ops.video_prep(src, None, 9, y0, x0, 5, 7, False, [], None, out, PAD)
    for bad in (9, -1):
        with pytest.raises(ValueError, match="frame index"):
            ops.video_prep(src, [0, 1, 2, 3, 4, 5, 6, 7, bad], 9, 0, 0, 5, 7, False, [], None, out, PAD)
    with pytest.raises(TavsrError, match="frame counts"):
        ops.video_prep(src, None, 10, 0, 0, 5, 7, False, [], None, torch.empty(10, 5, 7, device="cuda"), PAD)


# ------------------------------------------------------------------------------------------------ j. utterance_mvn
@pytest.mark.parametrize("T", [2000, 6000])
@pytest.mark.parametrize("Fq", [80, 81])
def test_utterance_mvn_of_a_near_constant_utterance(T, Fq):
    """F = 80: the vector kernel; F = 81: the scalar kernel, four threads per column, T / 4 rows each in sequence"""
    from tavsr import ops
    x = -23 + 0.01 * torch.randn(2, T, Fq, generator=_gen(T + Fq))
    lens = [T, T // 3]
    x[1, lens[1]:] = float("nan")
    want = R.utterance_mvn(x.double(), torch.tensor(lens))
    xd = x.cuda()
    got = ops.utterance_mvn(xd, _i64(lens)).cpu()
    assert bool((got[1, lens[1]:] == 0).all())
    ek = e32 = ref_max = 0.0
    for b, le in enumerate(lens):
        t32 = (xd[b, :le] - xd[b, :le].sum(0) / le).cpu()
        e32 = max(e32, float((t32.double() - want[b, :le]).abs().max()))
        ek = max(ek, float((got[b, :le].double() - want[b, :le]).abs().max()))
        ref_max = max(ref_max, float(want[b, :le].abs().max()))
    bound = max(1e-5 * ref_max, 4 * e32)
    print(f"mvn T={T:<5d} F={Fq} ({'vector' if Fq % 4 == 0 else 'scalar'} kernel)  kernel {ek:.2e}  e32 {e32:.2e}  ratio {ek / max(e32, 1e-30):7.2f}  "
          f"bound {bound:.1e}  {'ok' if ek <= bound else 'FAIL'}")
    assert ek <= bound, (ek, bound)

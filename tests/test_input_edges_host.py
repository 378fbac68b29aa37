"""Host (no GPU): the restatements of tests/input_ref.py against the oracle's own routines (oracle/leaves.py, oracle/data.py) run in
float64 - the reference of tests/test_gpu_input_edges.py has to be right before a kernel is measured against it."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import input_ref as R
from oracle import data as D
from oracle import leaves as L

TOL = 1e-12       # float64 against float64, other summation order

# (n_fft, win_length, hop, center, n_mels): the geometries of the device test
GEOMETRIES = [(512, 400, 160, True, 80), (400, 400, 160, True, 80), (64, 48, 20, True, 20), (30, 30, 7, False, 20)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=TOL):
    a, b = a.detach().double(), b.detach().double()
    return a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ frontend
@pytest.mark.parametrize("N,pad", [(257, 256), (2, 1), (5, 4), (40, 15), (300, 256)])
def test_reflect_index_map_is_torch_reflect_padding(N, pad):
    """N = pad + 1 is the shortest signal torch pads; every padded position is read through the index map"""
    x = torch.arange(N, dtype=torch.float64) * 3 + 1
    want = F.pad(x[None, None, :], (pad, pad), mode="reflect")[0, 0]
    got = torch.stack([x[R.reflect_index(j - pad, N)] for j in range(N + 2 * pad)])
    assert torch.equal(got, want)
    if N == pad + 1:                    # one sample fewer and torch refuses the padding
        with pytest.raises(RuntimeError):
            F.pad(x[None, None, :N - 1], (pad, pad), mode="reflect")


@pytest.mark.parametrize("n_fft,hop,center,N", [(512, 160, True, 257), (400, 160, True, 1000), (30, 7, False, 100), (600, 200, True, 1000),
                                                (512, 160, False, 512)])
def test_frames_are_the_index_map_times_the_window(n_fft, hop, center, N):
    g = _gen(N)
    wav, win = torch.randn(2, N, generator=g, dtype=torch.float64), torch.rand(n_fft, generator=g, dtype=torch.float64)
    fr = R.frames(wav, win, n_fft, hop, center)
    T, pad = R.n_frames(N, n_fft, hop, center), (n_fft // 2 if center else 0)
    assert fr.shape == (2, T, n_fft)
    for t in {0, T // 2, T - 1}:
        src = torch.tensor([R.reflect_index(t * hop + n - pad, N) for n in range(n_fft)])
        assert torch.equal(fr[:, t], wav[:, src] * win)


def test_mel_filterbank_rounds_to_the_oracle_filterbank():
    for n_fft, _, _, _, n_mels in GEOMETRIES:
        assert torch.equal(R.mel_filterbank(16000, n_fft, n_mels).float(), L.slaney_mel_filterbank(16000, n_fft, n_mels))


@pytest.mark.parametrize("n_fft,win,hop,center,n_mels", GEOMETRIES)
def test_logmel_matches_the_oracle_frontend_in_float64(n_fft, win, hop, center, n_mels):
    g = _gen(n_fft)
    wav = 0.1 * (2 * torch.rand(3, 4000, generator=g, dtype=torch.float64) - 1)
    lens = torch.tensor([4000, 3001, 1700])
    ref = L.DefaultFrontend(n_fft=n_fft, win_length=win, hop_length=hop, center=center, n_mels=n_mels).double()
    assert ref.melmat.dtype == torch.float64
    want, olens_want = ref(wav, lens)
    got, olens = R.logmel(wav, lens, 16000, n_fft, win, hop, center, n_mels, melmat=ref.melmat)
    assert torch.equal(olens, olens_want) and int(olens[0]) == want.shape[1] == R.n_frames(4000, n_fft, hop, center)
    assert _close(got, want)
    for b, le in enumerate(olens.tolist()):
        assert bool((got[b, le:] == 0).all()) and bool((got[b, :le] != 0).any())
    # the module's own float64 filterbank: the oracle's weights are these rounded to fp32 (6e-8 of a mel power, so of the log)
    own, _ = R.logmel(wav, lens, 16000, n_fft, win, hop, center, n_mels)
    assert float((own - want).abs().max()) <= 2e-7


# ------------------------------------------------------------------------------------------------ SpecAug
@pytest.mark.parametrize("T,window", [(16, 4), (50, 5), (11, 5)])
def test_time_warp_matches_the_oracle_with_the_draws_replayed(T, window):
    x = torch.randn(3, T, 7, generator=_gen(T), dtype=torch.float64)
    seen = set()
    for seed in range(12):
        torch.manual_seed(seed)
        want = L.time_warp(x, window=window)
        torch.manual_seed(seed)
        if T - window <= window:
            c = w = 0
        else:
            c = int(torch.randint(window, T - window, (1,))[0])
            w = int(torch.randint(c - window, c + window, (1,))[0]) + 1
        seen.add((c, w))
        got = R.time_warp(x, [c] * 3, [w] * 3, [T] * 3)
        assert _close(got, want)
    assert len(seen) > (1 if T > 2 * window else 0)


def test_time_warp_of_a_ragged_batch_is_the_oracle_on_each_utterance():
    """the oracle's SpecAug warps every utterance on its own frames and pads with 0; rows past an utterance are never read"""
    lens = torch.tensor([16, 11, 8, 16])
    x = torch.randn(4, 18, 5, generator=_gen(1), dtype=torch.float64)
    sa = L.SpecAug(apply_time_warp=True, time_warp_window=4, apply_freq_mask=False, apply_time_mask=False)
    torch.manual_seed(5)
    want, _ = sa(x, lens)
    torch.manual_seed(5)
    cs, ws = [], []
    for le in lens.tolist():
        if le - 4 <= 4:
            cs.append(0), ws.append(0)
            continue
        cs.append(int(torch.randint(4, le - 4, (1,))[0]))
        ws.append(int(torch.randint(cs[-1] - 4, cs[-1] + 4, (1,))[0]) + 1)
    assert cs[2] == 0 and all(c > 0 for c in cs[:2])
    xn = x.clone()
    for b, le in enumerate(lens.tolist()):
        xn[b, le:] = float("nan")
    got = R.time_warp(xn, cs, ws, lens)
    assert got.shape == (4, 18, 5) and _close(got[:, :16], want) and bool((got[:, 16:] == 0).all())
    assert torch.equal(got[2, :8], x[2, :8]) and bool((got[2, 8:] == 0).all())


@pytest.mark.parametrize("dim,D", [(1, 50), (2, 13)])
def test_specaug_mask_matches_the_oracle_with_the_same_bands(dim, D):
    x = torch.randn(2, 50, 13, generator=_gen(dim), dtype=torch.float64) + 3
    for seed in range(6):
        rng = (0, 6)
        torch.manual_seed(seed)
        want, _ = L.mask_along_axis(x, None, rng, dim=dim, num_mask=3)
        torch.manual_seed(seed)
        length = torch.randint(rng[0], rng[1], (2, 3))
        pos = torch.randint(0, max(1, D - int(length.max())), (2, 3))
        got = R.specaug_mask(x, pos, length) if dim == 2 else R.specaug_mask(x, None, None, pos, length)
        assert torch.equal(got, want)


def test_specaug_mask_band_edges():
    """a band of length 0 masks nothing, one ending at the axis' size masks its last element, one reaching past it stops there"""
    x = torch.ones(1, 4, 5, dtype=torch.float64)
    y = R.specaug_mask(x, torch.tensor([[1, 3, 4]]), torch.tensor([[0, 2, 9]]), torch.tensor([[0, 0]]), torch.tensor([[1, 1]]))
    assert y[0].tolist() == [[0.0] * 5] + [[1.0, 1.0, 1.0, 0.0, 0.0]] * 3
    assert torch.equal(R.specaug_mask(x), x)


# ------------------------------------------------------------------------------------------------ clip assembly, noise, MVN
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_video_prep_matches_the_oracle_transforms(dtype):
    g = _gen(2)
    raw = torch.randint(0, 256, (9, 11, 13), generator=g, dtype=torch.uint8)
    raw = raw if dtype == torch.uint8 else raw.float() + torch.rand(9, 11, 13, generator=g)
    tr = D.Compose([D.VideoSpeedRate(1.5), D.Normalise(0.0, 250.0), D.Normalise(D.MEAN, D.STD), D.TimeMasking(fps=2.0, max_frames=2),
                    D.CenterCrop((5, 7)), D.RandomHorizontalFlip(p=1.0)])
    index = list(map(int, np.linspace(start=0, stop=9, num=6, endpoint=False)))
    for seed in range(4):
        random.seed(seed)
        want = tr(raw.double())
        random.seed(seed)
        masked = np.zeros(6, dtype=bool)
        for _ in range(3):
            ln = random.randint(0, 2)
            if ln > 0:
                off = random.randint(0, 6 - ln)
                masked[off:off + ln] = True
        got = R.video_prep(raw, index, 6, 3, 3, 5, 7, True, [(0.0, 250.0), (D.MEAN, D.STD)], masked, 8, -1.0)
        assert _close(got[:6], want) and bool((got[6:] == -1.0).all())
    plain = R.video_prep(raw, None, 9, 0, 6, 11, 7, False, [], None, 9, -1.0)
    assert torch.equal(plain, raw.double()[:, :, 6:])
    assert bool((R.video_prep(raw, None, 0, 0, 0, 5, 7, False, [], None, 3, -1.0) == -1.0).all())


@pytest.mark.parametrize("n", [1, 7, 1025])
def test_add_noise_matches_the_oracle_formula(n):
    g = _gen(n)
    audio = (1e-3 * torch.randn(1, n, generator=g, dtype=torch.float64) + 0.2)
    noise = 100 * torch.randn(1, n, generator=g, dtype=torch.float64)
    want = D.AddNoise(noise, snr_target=5)(audio)
    assert _close(R.add_noise(audio, noise, 1.0 / (10 ** (5 / 10.0)) ** 0.5), want)


@pytest.mark.parametrize("F_", [80, 81])
def test_utterance_mvn_matches_the_oracle(F_):
    x = -23 + 0.01 * torch.randn(2, 200, F_, generator=_gen(F_), dtype=torch.float64)
    lens = torch.tensor([200, 66])
    want, _ = L.UtteranceMVN()(x, lens)
    xn = x.clone()
    xn[1, 66:] = float("nan")
    got = R.utterance_mvn(xn, lens)
    assert _close(got, want) and bool((got[1, 66:] == 0).all())
    assert float(got[0].mean(0).abs().max()) <= 1e-13

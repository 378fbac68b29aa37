"""Host side of the device mask draw (``mask_draw = "device"``): the C ABI entry, the model switch, and the DISTRIBUTION of
the restatement ``tests/mask_draw_ref.py`` - it is checked here, on the CPU, so that the GPU tests can compare the kernel with
the restatement bit for bit.

Bounds.  4096 utterances of 12 tokens from one fixed seed.  ``n`` is uniform on 1..12: Pearson's chi-square has 11 degrees of
freedom, and 37.37 is its 1 - 1e-4 quantile.  The number of utterances in which position p is masked has the same expectation
for every p and the positions are exchangeable, so the chi-square of the 12 counts against their common mean is, for 4096
utterances, a chi-square(11) variable times 1 - P(p' masked | p masked) < 1: the same bound holds with room.  The number of
distinct masked positions of a draw of n with replacement out of 12 has mean 12 (1 - (11/12)^n); averaged over n = 1..12
that is 4.872 (6.5 without replacement), and the sample mean is asked to be within 4 of its standard errors.  numpy's own
reference draw stays at chi-square <= 17.8 and <= 10.4 and |z| <= 2.7 over 20 seeds."""
import argparse
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mask_draw_ref as D
import maskctc_ref as R
from helpers import ROOT

CHI2_11_Q9999 = 37.37
SEED, OFFSET = 0x5EED5EED, 0       # fixed: chosen once as a seed the restatement passes with, never tuned afterwards
N_UTT, LEN = 4096, 12
MASK, EOS, IGN = 41, 40, -1


@pytest.fixture(scope="module")
def draw():
    rng = np.random.RandomState(0)
    text = rng.randint(1, 40, size=(N_UTT, LEN)).astype(np.int64)
    return (text,) + D.mask_uniform_dev_ref(text, MASK, EOS, IGN, SEED, OFFSET, with_n=True)


def test_philox_restatement_known_answers():
    """Random123's known-answer vector for philox4x32-10 (counter and key zero): the restatement is the published generator,
    with the 64-bit counter in counter words 0-1 and the 64-bit seed as the key"""
    assert D.philox4x32_10(0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert D.word(5, 0) == D.philox4x32_10(1, 0)[1]
    assert D.counters_per_row(12) == 16 and D.counters_per_row(3) == 4 and D.counters_per_row(4) == 8


def test_header_declares_the_entry_points_and_the_binding_reads_them():
    from tavsr import _lib
    hdr = open(os.path.join(ROOT, "include", "tavsr.h")).read()
    assert {"tavsr_mask_uniform", "tavsr_count_recip"} <= set(re.findall(r"\b(tavsr_[a-z0-9_]+)\s*\(", hdr))
    restype, args = _lib.PROTOTYPES["tavsr_mask_uniform"]
    assert restype is ctypes.c_int and len(args) == 14
    assert args[1] is ctypes.c_int64 and args[8] is ctypes.c_uint64 and args[2] is ctypes.c_int32
    assert _lib.ENUMS["TAVSR_MASK_UNIFORM_MAX_L"] >= 2048


def test_entry_point_validates_before_anything_is_launched():
    from tavsr import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, "tailored-avsr_amd", "tavsr", "lib", "libtavsr_hip.so"))
    lib.tavsr_last_error_string.restype = ctypes.c_char_p
    buf = (ctypes.c_int64 * 16)()                 # a host address: the checks return before anything is launched or read
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    i64, i32, u64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64
    lim = _lib.ENUMS["TAVSR_MASK_UNIFORM_MAX_L"]

    def call(text=p, seed=p, ys_in=p, L=4, ld_y=4, ld_text=4):
        return lib.tavsr_mask_uniform(text, i64(ld_text), i32(1), i32(L), i32(MASK), i32(EOS), i32(IGN), seed, u64(0), ys_in, p,
                                      i64(ld_y), null, null)

    cases = ((dict(text=null), -1, "null pointer"), (dict(seed=null), -1, "null pointer"), (dict(ys_in=null), -1, "null pointer"),
             (dict(ld_y=3), -1, "ld_y"), (dict(L=-1), -1, "Lmax"),
             (dict(L=lim + 1, ld_y=lim + 1, ld_text=lim + 1), _lib.ENUMS["TAVSR_EUNSUPPORTED"], "limit"))
    for kw, want, what in cases:
        rc = call(**kw)
        assert rc == want and what in lib.tavsr_last_error_string().decode(), (kw, rc, lib.tavsr_last_error_string())


def test_mask_draw_defaults_to_host_and_a_bad_value_raises():
    from tavsr.models.avsr_maskctc_model import AVSRMaskCTCModel
    from tavsr.models.maskctc_model import MaskCTCModel
    from tavsr.tasks.asr import ASRTask
    assert MaskCTCModel.mask_draw == "host" and AVSRMaskCTCModel.mask_draw == "host"
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(R.asr_maskctc_conf(num_blocks=1, dec_blocks=1))))
    assert model.mask_draw == "host" and model.last_mask_token is None
    model.mask_draw = "gpu"
    text = torch.tensor([[3, 4, 5]])
    with pytest.raises(ValueError, match="mask_draw"):
        model._decoder_branch(None, None, text, torch.tensor([3]))
    assert "mask_draw" not in model.state_dict()


def test_host_draw_under_capture_names_the_switch(monkeypatch):
    from tavsr.tasks.asr import ASRTask
    model = ASRTask.build_model(argparse.Namespace(**copy.deepcopy(R.asr_maskctc_conf(num_blocks=1, dec_blocks=1))))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)

    class DeviceText:      # (stands for a device tensor: the check comes before anything is read)
        is_cuda = True

    with pytest.raises(NotImplementedError, match='mask_draw = "device"'):
        model._decoder_branch(None, None, DeviceText(), None)


def test_ops_mask_uniform_refuses_cpu_tensors():
    from tavsr import ops
    from tavsr._lib import TavsrError
    with pytest.raises(TavsrError):
        ops.mask_uniform(torch.tensor([[3, 4, 5]]), MASK, EOS, IGN)


def test_restatement_n_is_uniform(draw):
    ns = draw[4]
    assert ns.min() == 1 and ns.max() == LEN
    obs = np.bincount(ns, minlength=LEN + 1)[1:]
    chi2 = float(((obs - N_UTT / LEN) ** 2 / (N_UTT / LEN)).sum())
    print("chi2(n) =", chi2)
    assert chi2 < CHI2_11_Q9999


def test_restatement_masks_every_position_alike(draw):
    ys_out = draw[2]
    obs = (ys_out != IGN).sum(axis=0)
    e = obs.sum() / LEN
    chi2 = float(((obs - e) ** 2 / e).sum())
    print("chi2(position) =", chi2)
    assert chi2 < CHI2_11_Q9999


def test_restatement_draws_with_replacement(draw):
    n_target = draw[3].astype(np.float64)
    want = np.mean([LEN * (1 - (1 - 1 / LEN) ** n) for n in range(1, LEN + 1)])
    assert abs(want - 4.872) < 5e-4
    se = n_target.std(ddof=1) / np.sqrt(N_UTT)
    z = (n_target.mean() - want) / se
    print("mean distinct =", n_target.mean(), "z =", z)
    assert abs(z) < 4
    assert abs(6.5 - want) / se > 4           # a draw without replacement would not pass


def test_restatement_invariants(draw):
    text, ys_in, ys_out, n_target, ns = draw
    masked = ys_out != IGN
    assert np.array_equal(ys_out[masked], text[masked])
    assert np.array_equal(ys_in == MASK, masked)
    assert np.array_equal(ys_in[~masked], text[~masked])
    assert np.array_equal(n_target, masked.sum(axis=1)) and n_target.min() >= 1 and n_target.max() <= LEN
    assert (n_target <= ns).all()
    # ragged rows, an ignore_id in the middle and an empty row: compaction and padding
    rag = np.array([[5, 6, 7, 8, IGN, IGN], [IGN, 9, IGN, 10, 11, IGN], [IGN] * 6, [12, IGN, IGN, IGN, IGN, IGN]])
    yi, yo, nt = D.mask_uniform_dev_ref(rag, MASK, EOS, IGN, SEED, 64)
    for b, toks in enumerate(([5, 6, 7, 8], [9, 10, 11], [], [12])):
        ln = len(toks)
        m = yo[b] != IGN
        assert not m[ln:].any() and (yi[b, ln:] == EOS).all()
        assert np.array_equal(yo[b][m], np.array(toks, dtype=np.int64)[m[:ln]])
        assert np.array_equal(yi[b, :ln], np.where(m[:ln], MASK, toks))
        assert nt[b] == m.sum() and (1 <= nt[b] <= ln if ln else nt[b] == 0)
    assert yi[3, 0] == MASK and yo[3, 0] == 12      # len = 1: n = 1 and the only position is masked

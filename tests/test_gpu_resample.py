"""The windowed-sinc resampling kernel (csrc/resample.hip, aed_resample_sinc) on the GPU: impulses against the bank bit for
bit, random clips against an fp64 FIR with the same fp32 bank under the fp32 dot-product bound, the device arm of
utils.resample against the host arm, load_audio end to end, and the refusal of a wrong out_len."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_reference as ref                                                           # noqa: E402
from audioeditingcode_amd import _lib as L                                                 # noqa: E402
from audioeditingcode_amd import utils                                                     # noqa: E402

DEV = "cuda:0"
BLOCK = 256                      # outputs per block of resample_sinc_kernel


def _kernel(x, orig, new):
    """x [C, L] float32 numpy -> y [C, out_len] through the C ABI."""
    bank, width, o, n = utils.sinc_resample_bank(orig, new)
    xd = torch.tensor(x, dtype=torch.float32, device=DEV)
    C, length = xd.shape
    out_len = ref.out_length(orig, new, length)
    bank_t = bank.t().contiguous().to(DEV)
    y = torch.full((C, out_len), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        L.check(L.lib().aed_resample_sinc(xd.data_ptr(), C, length, bank_t.data_ptr(), o, n, width, y.data_ptr(), out_len,
                                          L.current_stream_ptr()), "aed_resample_sinc")
        torch.cuda.synchronize()
    return y.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 5. impulses, bit-exact
@pytest.mark.parametrize("orig, new, shape, width", ref.RATE_PAIRS, ids=ref.PAIR_IDS)
def test_impulses_return_the_bank_bit_for_bit(orig, new, shape, width):
    """One 1.0 per channel at 0, L-1 and mid-clip: every output is one bank entry (products with 1.0 and sums with zeros
    are exact in any order) or zero -- any indexing, edge or phase error shows, the near-zero outer taps included."""
    length = 2000
    pos = [0, length - 1, length // 2 + 3]
    x = np.zeros((3, length), dtype=np.float32)
    x[np.arange(3), pos] = 1.0
    bank, w, o, n = utils.sinc_resample_bank(orig, new)
    bank = bank.numpy()
    taps = 2 * w + o
    j = np.arange(ref.out_length(orig, new, length))
    q, p = j // n, j % n
    want = np.zeros((3, len(j)), dtype=np.float32)
    for c in range(3):
        k = pos[c] - q * o + w                                   # the tap that meets the impulse in output j
        ok = (k >= 0) & (k < taps)
        want[c, ok] = bank[p[ok], k[ok]]
        assert ok.any()
    got = _kernel(x, orig, new)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_impulses_past_2_31_samples():
    """The only shape at which a 32-bit sample offset would show: one channel of 2^31 + 4096 samples, 48000 -> 16000 (3:1, one
    phase), impulses at 0, just past 2^31 and at L-1.  Every output a tap reaches equals its bank entry bit for bit; all the
    others are zero (counted on the device: the bank has no zero entry)."""
    length = 2 ** 31 + 4096
    bank, w, o, n = utils.sinc_resample_bank(48000, 16000)
    assert (o, n) == (3, 1) and int((bank == 0).sum()) == 0
    out_len = ref.out_length(48000, 16000, length)
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 4 * (length + out_len) + (2 << 30):
        pytest.skip(f"needs {4 * (length + out_len) >> 30} GiB of free device memory, {free >> 30} GiB are free")
    pos = [0, 2 ** 31 + 5, length - 1]
    x = torch.zeros(1, length, dtype=torch.float32, device=DEV)
    for p in pos:
        x[0, p] = 1.0
    y = torch.full((1, out_len), float("nan"), dtype=torch.float32, device=DEV)
    bank_t = bank.t().contiguous().to(DEV)
    with torch.cuda.device(DEV):
        L.check(L.lib().aed_resample_sinc(x.data_ptr(), 1, length, bank_t.data_ptr(), o, n, w, y.data_ptr(), out_len,
                                          L.current_stream_ptr()), "aed_resample_sinc")
        torch.cuda.synchronize()
    hits = 0
    for p in pos:
        q = np.arange(max(0, -(-(p + w - (2 * w + o) + 1) // o)), min(out_len - 1, (p + w) // o) + 1)      # 0 <= p - q*o + w < taps
        want = bank.numpy()[0, p - q * o + w]
        got = y[0, int(q[0]):int(q[-1]) + 1].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (p, got, want)
        hits += len(q)
    assert int(torch.count_nonzero(y)) == hits                           # a NaN left by an unwritten output counts too

# ------------------------------------------------------------------------------------------------ 6. random clips vs fp64
def _len_for(orig, new, out_len):
    """The shortest clip whose resampled length is out_len."""
    o, n, _, _ = ref.reduced(orig, new)
    length = (out_len - 1) * o // n + 1
    assert ref.out_length(orig, new, length) == out_len
    return length


RANDOM_CASES = [
    ("44100->16000 C2 L1500", 44100, 16000, 2, 1500),
    ("44100->16000 L5 (shorter than the width)", 44100, 16000, 1, 5),
    ("44100->16000 L1323 (3 o exactly)", 44100, 16000, 1, 1323),
    # out_len one short of, equal to and one past a block's outputs ...
    ("44100->16000 out_len 255", 44100, 16000, 1, _len_for(44100, 16000, BLOCK - 1)),
    ("44100->16000 out_len 256", 44100, 16000, 1, _len_for(44100, 16000, BLOCK)),
    ("44100->16000 out_len 257", 44100, 16000, 1, _len_for(44100, 16000, BLOCK + 1)),
    # ... and 255, 256 and 257 whole blocks
    ("44100->16000 out_len 255 blocks", 44100, 16000, 1, _len_for(44100, 16000, 255 * BLOCK)),
    ("44100->16000 out_len 256 blocks", 44100, 16000, 1, _len_for(44100, 16000, 256 * BLOCK)),
    ("44100->16000 out_len 257 blocks", 44100, 16000, 1, _len_for(44100, 16000, 257 * BLOCK)),
    ("16000->44100 C1 L700 (n = 441 > block)", 16000, 44100, 1, 700),
    ("48000->44100 C3 L900", 48000, 44100, 3, 900),
    ("48000->16000 C2 L1000 (n = 1)", 48000, 16000, 2, 1000),
    ("8000->16000 L300 (o = 1)", 8000, 16000, 1, 300),
]


@functools.lru_cache(maxsize=None)
def _random_case(orig, new, C, length):
    """(x, fp64 FIR with the product's fp32 bank, sum|K||x|, taps): computed once per shape, shared, never written to."""
    rng = np.random.default_rng(1000 * C + length)
    x = (0.4 + 0.3 * rng.standard_normal((C, length))).astype(np.float32)      # the common mode shows both zero-padded edges
    bank, width, o, n = utils.sinc_resample_bank(orig, new)
    want, mag = ref.fir_fp64(x, bank.numpy(), o, width, with_bound=True)
    for a in (x, want, mag):
        a.setflags(write=False)
    return x, want, mag, bank.shape[1]


@pytest.mark.parametrize("name, orig, new, C, length", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_random_clips_meet_the_fp32_dot_product_bound(name, orig, new, C, length):
    """|y - ref| <= gamma * sum_k |K||x| per element, gamma = taps*2^-24 / (1 - taps*2^-24): the bound of an fp32 dot
    product in any summation order (derived, not tuned; torch's CPU conv1d sits at 0.001 to 0.22 of it on these shapes)."""
    x, want, mag, taps = _random_case(orig, new, C, length)
    got = _kernel(x, orig, new)
    assert got.shape == want.shape == (C, ref.out_length(orig, new, length))
    ratio = np.abs(got - want) / (ref.gamma(taps) * mag)
    print(f"{name}: max |y - ref| / bound = {ratio.max():.3f}")
    assert np.isfinite(got).all() and (ratio <= 1.0).all()


# ------------------------------------------------------------------------------------------------ 7. host and device arms
@pytest.mark.parametrize("orig, new, C, length", [(44100, 16000, 2, 1500), (16000, 44100, 1, 700), (48000, 16000, 2, 1000)])
def test_device_arm_agrees_with_the_host_arm(orig, new, C, length):
    """Each arm is within the bound of test 6 of the fp64 FIR, so the two are within twice it of each other."""
    x, _, mag, taps = _random_case(orig, new, C, length)
    x = x.copy()
    host = utils.resample(x, orig, new, method="sinc")
    dev = utils.resample(x, orig, new, method="sinc", device=DEV)
    assert dev.dtype == np.float32 and dev.shape == host.shape == mag.shape
    assert (np.abs(dev - host) <= 2 * ref.gamma(taps) * mag).all()
    one = utils.resample(x[0], orig, new, method="sinc", device=torch.device(DEV))          # [L] in, [out_len] out
    assert one.shape == host.shape[1:] and np.array_equal(one, dev[0])


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_load_audio_end_to_end_with_the_device_resampler():
    """One second at 44.1 kHz through load_audio's mel branch with the resampler on the GPU against the same call with the host
    arm.  The two 16 kHz waveforms differ by at most twice the bound of test 6 (a few 1e-7 here), far inside what the STFT
    engine is itself held to against the reference's mel (tests/test_gpu_codec.py: atol 2e-3, rtol 1e-4) -- the bound on the
    mel.  Then the raw-waveform branch on a stereo 16 kHz clip: both channels in one launch."""
    from audioeditingcode_amd import models
    m = models.load_model("tiny/audioldm2", DEV, 4, seed=0)
    w44k = ref.tone_plus_noise(44100)
    mel_d, _, dur = utils.load_audio((w44k, 44100), m.get_fn_STFT(), stft=True, device=DEV, resampler="sinc")
    mel_h, _, _ = utils.load_audio((w44k, 44100), m.get_fn_STFT(), stft=True, device="cpu", resampler="sinc")
    assert dur == 1.0 and mel_d.shape == mel_h.shape == (1, 1, 102, 64) and mel_d.device.type == "cuda"
    np.testing.assert_allclose(mel_d.cpu().numpy(), mel_h.cpu().numpy(), atol=2e-3, rtol=1e-4)
    st = np.stack([ref.tone_plus_noise(16000, 0.25, seed=1), ref.tone_plus_noise(16000, 0.25, seed=2)])
    w_d, sr, d = utils.load_audio((st, 16000), None, stft=False, model_sr=44100, device=DEV, resampler="sinc")
    w_h, _, _ = utils.load_audio((st, 16000), None, stft=False, model_sr=44100, device="cpu", resampler="sinc")
    assert sr == 44100 and d == 0.25 and tuple(w_d.shape) == tuple(w_h.shape) == (2, 11025)
    # r_d, r_h: the two resampled pairs, |r_d - r_h| <= eps = 2 gamma max(sum|K||x|) (test 7).  The normalisation is
    # f(r) = 0.5 (r - mean r) / (P + 1e-8), P = max|r - mean r|: the mean moves by <= eps, the numerator and P by <= 2 eps, so
    # |f(r_d) - f(r_h)| <= 0.5 (2 eps / P + P * 2 eps / P^2) = 2 eps / P; the fp32 roundings of the mean, the subtraction, the
    # division and the product add a few ulp of the 0.5 peak on each side (8 * 2^-24 allowed).
    bank, width, o, n = utils.sinc_resample_bank(16000, 44100)
    r_h, mag = ref.fir_fp64(st, bank.numpy(), o, width, with_bound=True)
    eps = 2 * ref.gamma(bank.shape[1]) * mag.max()
    peak = np.abs(r_h - r_h.mean()).max()
    assert (w_d - w_h).abs().max().item() <= 2 * eps / peak + 8 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 9. the error path
def test_wrong_out_len_is_refused_before_any_launch():
    bank, width, o, n = utils.sinc_resample_bank(44100, 16000)
    x = torch.zeros(1, 1500, device=DEV)
    bank_t = bank.t().contiguous().to(DEV)
    y = torch.full((1, 546), 7.0, device=DEV)
    lib = L.lib()
    for out_len in (544, 546):
        rc = lib.aed_resample_sinc(x.data_ptr(), 1, 1500, bank_t.data_ptr(), o, n, width, y.data_ptr(), out_len,
                                   L.current_stream_ptr())
        assert rc != 0 and b"expected ceil(160*1500/441) = 545" in lib.aed_last_error(), lib.aed_last_error()
    torch.cuda.synchronize()
    assert (y == 7.0).all()                                              # nothing ran
    with pytest.raises(L.AedError, match="out_len"):
        L.check(rc, "aed_resample_sinc")

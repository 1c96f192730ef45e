"""Audio I/O + helpers mirroring the reference's code/utils.py (load_audio :53-95, get_spec :49-50,
set_reproducability :98-116, get_text_embeddings :217-231) and audioldm/audio/tools.py
(normalize_wav :46-49, pad_wav :34-44, read_wav_file :52-64, _pad_spec :18-31, wav_to_fbank :67-85), and the
resampler both call (torchaudio.functional.resample at its defaults), restated: sinc_resample_bank / resample(method="sinc")."""
import math
import random
import wave
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch


class PromptEmbeddings(NamedTuple):           # pc_drift.py:10-13
    embedding_hidden_states: torch.Tensor
    embedding_class_lables: torch.Tensor
    boolean_prompt_mask: torch.Tensor


def normalize_wav(waveform):
    waveform = waveform - np.mean(waveform)
    waveform = waveform / (np.max(np.abs(waveform)) + 1e-8)
    return waveform * 0.5


def pad_wav(waveform, segment_length):
    n = waveform.shape[-1]
    assert n > 100, "Waveform is too short, %s" % n
    if segment_length is None or n == segment_length:
        return waveform
    if n > segment_length:
        # the reference slices the FIRST axis of the [1, N] array here (tools.py:39-40): a no-op, the waveform is not
        # cropped and the surplus frames are cut by _pad_spec; kept as is (pinned by tests/golden/waveform_prep.npz)
        return waveform[:segment_length]
    tmp = np.zeros((1, segment_length))          # float64 like the reference
    tmp[:, :n] = waveform
    return tmp


def prepare_waveform(waveform_16k, segment_length):
    """read_wav_file after loading/resampling: normalise, pad/crop, normalise AGAIN (tools.py:57,61-62)."""
    w = normalize_wav(np.asarray(waveform_16k))[None, ...]
    w = pad_wav(w, segment_length)
    w = w / np.max(np.abs(w))
    return (0.5 * w)[0].astype(np.float32)


def read_wav(path) -> Tuple[np.ndarray, int]:
    """Mono float waveform + sample rate: channel 0 of `read_wav_channels`, as the reference's `numpy()[0]` (tools.py:54)."""
    w, sr = read_wav_channels(path)
    return w[0], sr


def read_wav_channels(path) -> Tuple[np.ndarray, int]:
    """[channels, n] float waveform + sample rate (`torchaudio.load`'s layout, utils.py:78)."""
    try:
        import torchaudio
        w, sr = torchaudio.load(path)
        return w.numpy(), sr
    except ImportError:
        with wave.open(path, "rb") as f:
            sr, nch, sw, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            raw = f.readframes(n)
        if sw == 1:                                     # 8-bit PCM is unsigned, centred on 128
            x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        elif sw == 3:                                   # 24-bit little-endian: widen to int32 (sign in the top byte)
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            x = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8 >> 8).astype(np.float32) / float(1 << 23)
        elif sw in (2, 4):
            dt = {2: np.int16, 4: np.int32}[sw]
            x = np.frombuffer(raw, dtype=dt).astype(np.float32) / float(np.iinfo(dt).max + 1)
        else:
            raise ValueError(f"{path}: unsupported PCM sample width {sw} bytes (torchaudio is not installed)")
        return np.ascontiguousarray(x.reshape(-1, nch).T), sr


SINC_BANK_LIMIT = 64 << 20          # bytes of one filter bank `sinc_resample_bank` still builds


def sinc_resample_bank(orig: int, new: int):
    """The filter bank of `torchaudio.functional.resample(w, orig, new)` at its defaults (sinc_interp_hann,
    lowpass_filter_width 6, rolloff 0.99), restated from `_get_sinc_resample_kernel`: torch fp32 ops in torchaudio's own
    order, so the bank is the one torchaudio computes for an fp32 waveform.  Returns (bank fp32 [n, taps], width, o, n) with
    o, n the reduced rates and taps = 2*width + o (include/aed.h, aed_resample_sinc, has the closed form)."""
    orig, new = int(orig), int(new)
    if orig <= 0 or new <= 0:
        raise ValueError(f"sample rates must be positive, got {orig} -> {new}")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    lowpass_filter_width, rolloff = 6, 0.99
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    size = 4 * n * (2 * width + o)
    if size > SINC_BANK_LIMIT:
        raise ValueError(f"resampling {orig} -> {new} Hz reduces to the ratio {o}:{n}, whose sinc filter bank "
                         f"([{n}, {2 * width + o}] fp32, {size / 2 ** 20:.0f} MiB) is over the {SINC_BANK_LIMIT >> 20} MiB limit")
    idx = torch.arange(-width, width + o, dtype=torch.float32)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float32)[:, None, None] / n + idx
    t *= base
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels[:, 0], width, o, n


def _resample_sinc(w, sr, new_sr, device):
    """[channels, L] or [L] float32 -> same rank at the new rate.  On a GPU device: csrc/resample.hip, all channels in one
    launch.  Otherwise torchaudio's own CPU op sequence (`_apply_sinc_resample_kernel`: pad, conv1d with stride o, cut)."""
    bank, width, o, n = sinc_resample_bank(sr, new_sr)
    x = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
    x2 = x.reshape(-1, x.shape[-1])
    channels, length = x2.shape
    out_len = -(-n * length // o)
    if device is not None and torch.device(device).type == "cuda":
        from . import _lib as L
        with torch.cuda.device(device):
            xd = x2.to(device)
            bank_t = bank.t().contiguous().to(device)
            y = torch.empty(channels, out_len, dtype=torch.float32, device=device)
            L.check(L.lib().aed_resample_sinc(xd.data_ptr(), channels, length, bank_t.data_ptr(), o, n, width, y.data_ptr(),
                                              out_len, L.current_stream_ptr()), "aed_resample_sinc")
            y = y.cpu()
    else:
        xp = torch.nn.functional.pad(x2, (width, width + o))
        y = torch.nn.functional.conv1d(xp[:, None], bank[:, None], stride=o)
        y = y.transpose(1, 2).reshape(channels, -1)[..., :out_len]
    return y.reshape(x.shape[:-1] + (out_len,)).numpy()


def resample(w, sr, new_sr, method=None, device=None):
    """`method=None`: torchaudio when it is installed, else scipy's polyphase resampler (a different filter: a stand-in).
    `method="sinc"`: the native restatement of torchaudio's default resampler (`sinc_resample_bank`), on the HIP kernel when
    `device` is a GPU device and in host torch otherwise; takes [L] or [channels, L].  Returns float32 numpy."""
    if sr == new_sr:
        return w
    if method == "sinc":
        return _resample_sinc(w, sr, new_sr, device)
    if method is not None:
        raise ValueError(f"unknown resampling method {method!r} (None or 'sinc')")
    try:
        import torchaudio
        return torchaudio.functional.resample(torch.from_numpy(w)[None], orig_freq=sr, new_freq=new_sr)[0].numpy()
    except ImportError:
        from scipy.signal import resample_poly
        g = math.gcd(sr, new_sr)
        return resample_poly(w, new_sr // g, sr // g).astype(np.float32)


def resampler_label(src, target_sr, resampler=None):
    """Which resampler `load_audio(src, ..., resampler=resampler)` runs for a clip (a path or a (waveform, rate) pair) that
    has to end at `target_sr`: the line the CLIs print next to the weight and conditioning sources."""
    if isinstance(src, str):
        with wave.open(src, "rb") as f:
            sr = f.getframerate()
    else:
        sr = src[1]
    if sr == target_sr:
        return "none: already at the model rate"
    if resampler == "sinc":
        return "sinc (native)"
    try:
        import torchaudio  # noqa: F401
        return "torchaudio"
    except ImportError:
        return "scipy polyphase stand-in"


def get_duration(path):
    with wave.open(path, "rb") as f:           # audioldm/utils.py:17-21
        return f.getnframes() / float(f.getframerate())


def pad_spec(fbank, target_length=1024):
    n = fbank.shape[0]
    p = target_length - n
    if p > 0:
        fbank = torch.nn.functional.pad(fbank, (0, 0, 0, p))
    elif p < 0:
        fbank = fbank[0:target_length, :]
    if fbank.size(-1) % 2 != 0:
        fbank = fbank[..., :-1]
    return fbank


def wav_to_fbank(waveform_16k, target_length, fn_STFT):
    """In-memory waveform -> (fbank [target_length, n_mels] on the STFT's device, waveform tensor)."""
    w = torch.from_numpy(prepare_waveform(waveform_16k, target_length * 160))
    mel, _, _ = fn_STFT.mel_spectrogram(torch.clip(w[None], -1, 1))
    fbank = pad_spec(mel[0].T, target_length)
    return fbank, w


def get_spec(wav: torch.Tensor, fn_STFT) -> torch.Tensor:
    return fn_STFT.mel_spectrogram(torch.clip(wav[:, 0], -1, 1).cpu())[0]


def load_audio(audio_path, fn_STFT, left: int = 0, right: int = 0, device: Optional[torch.device] = None,
               return_wav: bool = False, stft: bool = False, model_sr: Optional[int] = None,
               resampler: Optional[str] = None):
    """code/utils.py:53-95: the AudioLDM/TANGO spectrogram branch (stft=True) and the Stable Audio raw-waveform branch
    (stft=False -> (waveform [channels, n] normalised to +-0.5 over all channels, model_sr, duration)).  `audio_path` may
    also be a (waveform, sample_rate) pair for in-memory clips.  `resampler` is `resample`'s `method` (None: as before;
    "sinc": the native restatement of torchaudio's resampler, on `device` when that is a GPU)."""
    if not stft:
        if isinstance(audio_path, str):
            wav, sr = read_wav_channels(audio_path)
        else:
            wav, sr = audio_path
            wav = np.asarray(wav, dtype=np.float32)
            wav = wav[None] if wav.ndim == 1 else wav
        if sr != model_sr:
            if resampler is None:
                wav = np.stack([resample(c, sr, model_sr) for c in wav])
            else:
                wav = resample(wav, sr, model_sr, method=resampler, device=device)     # all channels in one call
        w = torch.from_numpy(np.ascontiguousarray(wav)).float()
        w = w - torch.mean(w)                                   # utils.py:83-88
        w = w / (torch.max(torch.abs(w)) + 1e-8)
        w = w * 0.5
        return w, model_sr, w.shape[-1] / model_sr
    if isinstance(audio_path, str):
        wav, sr = read_wav(audio_path)
        duration = get_duration(audio_path)
    elif isinstance(audio_path, tuple):
        wav, sr = audio_path
        duration = len(wav) / float(sr)
    else:
        mel, duration, wav = audio_path, None, None
    if wav is not None:
        wav16 = resample(np.asarray(wav, dtype=np.float32), sr, 16000, method=resampler, device=device)
        fbank, wav_t = wav_to_fbank(wav16, target_length=int(duration * 102.4), fn_STFT=fn_STFT)
        mel = fbank.unsqueeze(0)
    c, h, w = mel.shape
    left = min(left, w - 1)
    right = min(right, w - left - 1)
    mel = mel[:, :, left:w - right]
    mel = mel.unsqueeze(0).to(device)
    if return_wav:
        return mel, 16000, duration, wav_t
    return mel, model_sr, duration


def set_reproducability(seed: int, extreme: bool = True) -> None:
    if seed is not None:
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        random.seed(seed)
        np.random.seed(seed)


def get_text_embeddings(target_prompt: List[str], target_neg_prompt: List[str], ldm_stable):
    a = ldm_stable.encode_text(target_prompt)
    b = ldm_stable.encode_text(target_neg_prompt)
    text_emb = PromptEmbeddings(embedding_hidden_states=a[0], boolean_prompt_mask=a[2], embedding_class_lables=a[1])
    uncond_emb = PromptEmbeddings(embedding_hidden_states=b[0], boolean_prompt_mask=b[2], embedding_class_lables=b[1])
    return a[1], text_emb, uncond_emb


def write_wav(path, wav, sr=16000):
    """16-bit PCM.  wav: [n] (mono) or [channels, n] (the layout `torchaudio.save` takes in main_run.py:223-224; the
    Stable Audio path hands over [2, n]) -- channels are interleaved frame by frame, none is dropped."""
    x = np.clip(np.asarray(wav, dtype=np.float32), -1, 1)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError(f"write_wav expects [n] or [channels, n], got shape {x.shape}")
    with wave.open(path, "wb") as f:
        f.setnchannels(x.shape[0])
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(np.ascontiguousarray((x * 32767.0).astype(np.int16).T).tobytes())


def synthetic_clip(seconds=10.0, sr=16000, seed=1234):
    """SURVEY 8(d) synthetic benchmark clip: 100->4000 Hz chirp + 0.05 randn (CPU generator)."""
    n = int(seconds * sr)
    g = torch.Generator().manual_seed(seed)
    tt = torch.arange(n, dtype=torch.float64) / sr
    dur = n / sr
    phase = 2 * math.pi * (100.0 * tt + 0.5 * (4000.0 - 100.0) / dur * tt * tt)
    return (0.5 * torch.sin(phase).float() + 0.05 * torch.randn(n, generator=g)).numpy()

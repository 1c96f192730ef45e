"""Scores for written edits from the two CLAP towers: the cosine between a clip and a prompt (the CLAP score the paper behind the
reference reports, `evals/meta_clap_consistency.py`) and a perceptual distance between two clips over the audio tower's stage
outputs (the formula of `evals/lpaps.py`).  `ClapScorer` holds a text module (`clap.NativeClapModel` or a torch `ClapModel`),
an audio module (`clap_audio.NativeClapAudio` or a torch `ClapModel` / `ClapAudioModelWithProjection`), the tokenizer and the
feature extractor.  The tokenizer and the feature extractor (numpy: a 48 kHz power spectrogram in dB) stay on transformers and
run on the host.

Resampling to the extractor's rate is `utils.resample(method="sinc")`, the native restatement of torchaudio's windowed-sinc
filter -- not the julius filter of the reference's evaluation code: scores agree with the paper's tooling to the extent the two
resamplers do."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from . import utils
from .clap import NativeClapModel
from .clap_audio import NativeClapAudio


def lpaps(stages0, stages1):
    """The distance of `evals/lpaps.py` on two sets of stage outputs (lists of [B, L_i, C_i] tensors, one per stage): per stage
    unit-normalise over dim 1, square the difference, sum over dim 1, take the mean over what is left; then sum over the
    stages.  Returns [B].  The paper's LPAPS runs this formula on a laion-format HTSAT-base checkpoint
    (music_speech_epoch_15_esc_89.25), which this project does not load: the value here is the same distance on whatever
    Hugging Face checkpoint the scorer was given, and is comparable only between runs over that checkpoint."""
    if len(stages0) != len(stages1) or not stages0:
        raise L.AedError(f"lpaps: {len(stages0)} and {len(stages1)} stage outputs (need the same positive number)")
    val = 0
    for a, b in zip(stages0, stages1):
        a = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
        b = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
        val = val + ((a - b) ** 2).sum(dim=1, keepdim=True).mean(dim=[1, 2])
    return val


class ClapScorer:
    SEED = 0                # of the feature extractor's random truncation of a clip longer than its window

    def __init__(self, text, audio, tokenizer, feature_extractor, device=None):
        self.text, self.audio, self.tokenizer, self.feature_extractor = text, audio, tokenizer, feature_extractor
        if device is None:
            device = audio.engine.device if isinstance(audio, NativeClapAudio) else next(audio.parameters()).device
        self.device = torch.device(device)

    @property
    def towers(self):
        """Which implementation each tower runs, for the line the command-line tool prints."""
        return dict(text="native (op tape)" if isinstance(self.text, NativeClapModel) else "torch (transformers)",
                    audio="native (op tape)" if isinstance(self.audio, NativeClapAudio) else "torch (transformers)")

    @classmethod
    def from_pretrained(cls, root, device, text="native", audio="native"):
        """From a local directory, never the network: an AudioLDM2 snapshot (`text_encoder/` holding a ClapModel, `tokenizer/`,
        `feature_extractor/`) or a plain CLAP checkpoint directory that holds all three."""
        for name, v in (("text", text), ("audio", audio)):
            if v not in ("native", "torch"):
                raise L.AedError(f"ClapScorer: {name}={v!r} is not one of 'native', 'torch'")
        if not os.path.isdir(root):
            raise L.AedError(f"ClapScorer: {root} is not a directory (checkpoints are read from disk only)")
        snapshot = os.path.isdir(os.path.join(root, "text_encoder"))
        clap_dir = os.path.join(root, "text_encoder") if snapshot else root
        tok_dir = os.path.join(root, "tokenizer") if snapshot else root
        fe_dir = os.path.join(root, "feature_extractor") if snapshot else root
        from transformers import AutoTokenizer, ClapFeatureExtractor
        torch_model = None
        if "torch" in (text, audio):
            from transformers import ClapModel
            torch_model = ClapModel.from_pretrained(clap_dir, local_files_only=True).to(device).eval()
        text_mod = NativeClapModel.from_pretrained(clap_dir, device) if text == "native" else torch_model
        audio_mod = NativeClapAudio.from_pretrained(clap_dir, device) if audio == "native" else torch_model
        return cls(text_mod, audio_mod, AutoTokenizer.from_pretrained(tok_dir, local_files_only=True),
                   ClapFeatureExtractor.from_pretrained(fe_dir, local_files_only=True), device)

    # ------------------------------------------------------------------ audio
    def features(self, waveforms, sr):
        """Mono mix-down, resampling to the extractor's rate and the extractor itself (seeded): `input_features` [B, 1, T, F]."""
        rate = int(self.feature_extractor.sampling_rate)
        clips = []
        for w in waveforms:
            w = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float32)
            if w.ndim == 2:
                w = w.mean(0)
            if w.ndim != 1 or w.size == 0:
                raise L.AedError(f"ClapScorer: a waveform must be [n] or [channels, n], got {w.shape}")
            clips.append(np.asarray(utils.resample(w, int(sr), rate, method="sinc", device=self.device), dtype=np.float32))
        state = np.random.get_state()
        np.random.seed(self.SEED)
        try:
            feats = self.feature_extractor(clips, sampling_rate=rate, truncation="rand_trunc", return_tensors="pt")
        finally:
            np.random.set_state(state)
        return feats["input_features"].to(torch.float32)

    @torch.no_grad()
    def audio_forward(self, input_features, stages=False):
        """(`audio_embeds` [B, pd], stage outputs or None) of either kind of audio module; is_longer is not passed on (it only
        matters to fused checkpoints, which neither the native tower nor this scorer supports)."""
        if isinstance(self.audio, NativeClapAudio):
            out = self.audio(input_features, output_hidden_states=stages)
            return out.audio_embeds, (list(out.hidden_states) if stages else None)
        p = next(self.audio.parameters())
        ao = self.audio.audio_model(input_features=input_features.to(p.device, p.dtype), output_hidden_states=stages)
        emb = self.audio.audio_projection(ao.pooler_output)
        return emb, ([h.flatten(2).transpose(1, 2) for h in ao.hidden_states[1:]] if stages else None)

    def embed_audio(self, waveforms, sr, stages=False):
        """L2-normalised audio embeddings [B, pd] of waveforms ([n] or [channels, n] each) at rate `sr`; with `stages` also the
        tower's stage outputs (what `lpaps` takes)."""
        emb, st = self.audio_forward(self.features(waveforms, sr), stages)
        emb = F.normalize(emb.float(), dim=-1)
        return (emb, st) if stages else emb

    # ------------------------------------------------------------------ text
    @torch.no_grad()
    def embed_text(self, prompts):
        """L2-normalised text embeddings [B, pd]."""
        batch = self.tokenizer(list(prompts), padding=True, return_tensors="pt")
        ids, mask = batch.input_ids, batch.attention_mask
        if not isinstance(self.text, NativeClapModel):
            dev = next(self.text.parameters()).device
            ids, mask = ids.to(dev), mask.to(dev)
        out = self.text.get_text_features(input_ids=ids, attention_mask=mask)
        return F.normalize(getattr(out, "pooler_output", out).float(), dim=-1)

    # ------------------------------------------------------------------ scores
    def clap_score(self, waveforms, sr, prompts):
        """The cosine between clip k and prompt k, [B]: what `evals/meta_clap_consistency.py` averages."""
        prompts = list(prompts)
        if len(prompts) != len(waveforms):
            raise L.AedError(f"ClapScorer: {len(waveforms)} waveforms and {len(prompts)} prompts (need one prompt per clip)")
        a, t = self.embed_audio(waveforms, sr), self.embed_text(prompts)
        return F.cosine_similarity(a, t.to(a.device), dim=1, eps=1e-8)

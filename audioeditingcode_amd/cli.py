"""What the main_*.py scripts share: the options several of them take, the opening sequence (seed, device, model, clip),
the provenance fragment of their summary line, their post-parse checks and the results tail (one wav per record and a JSON
manifest).  Plain functions; a script keeps its own options, checks, library call, summary sentence and manifest header.

load_model, load_audio, synthetic_clip and the rest are reached through their home modules at call time, so a test that
replaces `models.load_model` or `utils.load_audio` replaces them for every script."""
import json
import os

import torch

from . import models, utils


def add_options(parser, *groups, model_id="cvssp/audioldm2-music", results_path="results", init_aud_help=None,
                scalar_cfg_src=False):
    """Declare the shared options of the named groups on `parser`, in the order given (the order --help lists them in; a
    script that has options of its own in between calls this more than once).  The keyword arguments are the differences
    between scripts: the defaults of --model_id and --results_path, the help of --init_aud, and --cfg_src taking one value
    instead of one per source prompt."""
    for group in groups:
        if group == "device":
            parser.add_argument("--device_num", type=int, default=0)
            parser.add_argument("-s", "--seed", type=int, default=None)
        elif group == "model":
            parser.add_argument("--model_id", type=str, default=model_id)
        elif group == "clip":
            parser.add_argument("--init_aud", type=str, default=None, help=init_aud_help)
        elif group == "cfg_src" and scalar_cfg_src:
            parser.add_argument("--cfg_src", type=float, default=3)
        elif group == "cfg_src":
            parser.add_argument("--cfg_src", type=float, nargs="+", default=[3])
        elif group == "steps":
            parser.add_argument("--num_diffusion_steps", type=int, default=200)
        elif group == "eta":
            parser.add_argument("--eta", type=float, default=1.0)
        elif group == "schedule":
            parser.add_argument("--schedule", default="sequential", choices=["sequential", "batched"])
        elif group == "results":
            parser.add_argument("--results_path", default=results_path)
        elif group == "synthetic":
            parser.add_argument("--allow_synthetic", action="store_true",
                                help="run with seeded-random weights / stand-in text embeddings when no checkpoint is on "
                                     "disk (benchmarking only: the output is noise)")
        elif group == "text_t5":
            parser.add_argument("--text_t5", default="torch", choices=["torch", "native"],
                                help="T5 text encoder: torch = transformers.T5EncoderModel, native = the encoder stack on "
                                     "the op tape (HIP kernels, one hipGraph per prompt batch shape); no effect with "
                                     "stand-in conditioning")
        elif group == "resampler":
            parser.add_argument("--resampler", default="auto", choices=["auto", "sinc"],
                                help="auto: torchaudio when installed, else scipy's polyphase stand-in; sinc: the native "
                                     "restatement of torchaudio's default resampler (HIP kernel)")
        else:
            raise ValueError(f"add_options: no option group {group!r}")


def require_family(parser, model_id, stable_audio, message):
    """Refuse (parser.error) a --model_id of the other kind: `stable_audio` says which kind the script's loop takes."""
    if ("stable-audio" in model_id) != stable_audio:
        parser.error(message)


def check_tstarts(parser, values, T):
    bad = [t for t in values if not 1 <= t <= T]
    if bad:
        parser.error(f"--tstart {bad} outside [1, --num_diffusion_steps={T}]")


def open_model(seed, device_num, model_id, num_diffusion_steps, double_precision=None, allow_synthetic=False, text_t5=None):
    """Seed, select the device, load the model: in this order, since synthetic weights and stand-in conditioning are
    seeded.  `double_precision` and `text_t5` reach load_model only when given.  Returns (model, device string)."""
    utils.set_reproducability(seed, extreme=False)
    device = f"cuda:{device_num}"
    torch.cuda.set_device(device_num)
    args = (model_id, device, num_diffusion_steps) + (() if double_precision is None else (double_precision,))
    kw = {} if text_t5 is None else dict(text_t5=text_t5)
    return models.load_model(*args, allow_synthetic=allow_synthetic or None, **kw), device


def load_clip(model, init_aud, device, resampler, stft, seed=None):
    """The clip a script edits: the wav at `init_aud`, or without one the synthetic 10 s clip (`seed`: the batch scripts'
    per-clip seed).  stft: the mel families' spectrogram (True) or Stable Audio's waveform (False).  Returns load_audio's
    (x0, sample rate, duration) and the resampler label of the summary line."""
    src = init_aud if init_aud else (utils.synthetic_clip() if seed is None else utils.synthetic_clip(seed=seed), 16000)
    method = None if resampler == "auto" else resampler
    x0, sr, duration = utils.load_audio(src, model.get_fn_STFT(), device=device, stft=stft, model_sr=model.get_sr(),
                                        resampler=method)
    return x0, sr, duration, utils.resampler_label(src, 16000 if stft else model.get_sr(), method)


def provenance(model, labels=None):
    """Where the weights and the text conditioning came from and, with `labels` (one resampler label or several), which
    resamplers ran: the fragment every script prints, so that a synthetic run is never mistaken for a real one."""
    text = f"weights: {model.weights_source}; text conditioning: {model.conditioning_source}"
    if labels is None:
        return text
    return text + f"; resampler: {', '.join(sorted(set([labels] if isinstance(labels, str) else labels)))}"


def vocode(model, latent, one_by_one=False):
    """Latents -> waveforms of a mel family: VAE decode (one_by_one: every row as a batch of one, as the PC drift scripts
    decode) and vocoder."""
    with torch.inference_mode():
        mel = torch.cat([model.vae_decode(w.unsqueeze(0)) for w in latent]) if one_by_one else model.vae_decode(latent)
        if mel.dim() < 4:
            mel = mel[None]
        return model.decode_to_mel(mel)


def prompt_dir(results_path, model_id, init_aud, prompts, neg_prompts):
    """results_path/<model>/<clip>/pmt_<prompts>__neg__<negative prompts>, created: where the reference's SDEdit and PC
    extraction scripts write."""
    clip = os.path.basename(init_aud).split(".")[0] if init_aud else "synthetic"
    path = os.path.join(results_path, model_id.split("/")[-1], clip,
                        "pmt_" + "__".join(x.replace(" ", "_") for x in prompts) + "__neg__" +
                        "__".join(x.replace(" ", "_") for x in neg_prompts))
    os.makedirs(path, exist_ok=True)
    return path


def write_rows(results_path, records, audio, sr, json_name, manifest):
    """The results tail: audio[k] ([n], [1, n] or stereo [2, n]) goes to results_path/records[k]["file"], and `manifest`
    (the script's header fields and the records, in the key order the script gives them) to results_path/json_name."""
    os.makedirs(results_path, exist_ok=True)
    for rec, wav in zip(records, audio):
        utils.write_wav(os.path.join(results_path, rec["file"]), wav.reshape(-1, wav.shape[-1]).numpy(), sr=sr)
    with open(os.path.join(results_path, json_name), "w") as f:
        json.dump(manifest, f, indent=1)

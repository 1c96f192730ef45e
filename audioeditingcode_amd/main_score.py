"""Score the wavs a batched edit script wrote: CLAP similarity to each edit's target prompt, and LPAPS to the source clip.

python -m audioeditingcode_amd.main_score --results DIR --clap PATH [--json NAME] [--source WAV] \
       [--text_clap native|torch] [--audio_clap native|torch]
Reads the manifest `cli.write_rows` wrote to DIR (--json, or the first of variants.json, grid.json, batch.json, segments.json
that exists), scores every record's `file` against its `target_prompt` in batches and writes scores.json beside the manifest:
one record per input record (index, file, clap and, with --source, lpaps) in input order, and the ranking (record indices,
best CLAP score first) as a second list.  --clap is a local AudioLDM2 snapshot or CLAP checkpoint directory."""
import argparse
import json
import os

import torch

from . import utils

MANIFESTS = ("variants.json", "grid.json", "batch.json", "segments.json")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--results", type=str, required=True, help="the --results_path of the script that wrote the edits")
    p.add_argument("--clap", type=str, required=True,
                   help="local AudioLDM2 snapshot (text_encoder/, tokenizer/, feature_extractor/) or CLAP checkpoint directory")
    p.add_argument("--json", type=str, default=None, help=f"the manifest's name (default: the first of {', '.join(MANIFESTS)})")
    p.add_argument("--source", type=str, default=None, help="the unedited clip: adds an LPAPS distance to it per edit")
    p.add_argument("--text_clap", type=str, default="native", choices=["native", "torch"])
    p.add_argument("--audio_clap", type=str, default="native", choices=["native", "torch"])
    p.add_argument("--batch", type=int, default=8, help="clips per forward pass of the audio tower")
    p.add_argument("--device_num", type=int, default=0)
    args = p.parse_args(argv)
    if args.batch < 1:
        p.error(f"--batch {args.batch} must be positive")
    return args


def find_manifest(results, name=None):
    """The manifest's path: `name` when given, else the first of MANIFESTS that exists in `results`."""
    for n in ((name,) if name else MANIFESTS):
        path = os.path.join(results, n)
        if os.path.isfile(path):
            return path
    raise FileNotFoundError(f"{results}: no manifest ({name or ', '.join(MANIFESTS)})")


def read_records(path):
    """The records of a manifest: its one list of objects that each name a `file`.  A record's `target_prompt` may be a list
    (one prompt per segment), which is joined with ', '."""
    with open(path) as f:
        manifest = json.load(f)
    for v in (manifest.values() if isinstance(manifest, dict) else [manifest]):
        if isinstance(v, list) and v and all(isinstance(r, dict) and "file" in r for r in v):
            for r in v:
                if "target_prompt" not in r:
                    raise ValueError(f"{path}: record {r.get('index', '?')} has no target_prompt")
            return v
    raise ValueError(f"{path}: no list of records with a `file` each")


def prompt_of(record):
    t = record["target_prompt"]
    return t if isinstance(t, str) else ", ".join(str(x) for x in t)


def score_records(scorer, results, records, source=None, batch=8):
    """(scores, ranking): one dict(index, file, clap[, lpaps]) per record in input order, and the positions of the records from
    the best CLAP score to the worst (ties keep input order).  Clips are read with all their channels (the Stable Audio scripts
    write stereo) and mixed down by the scorer."""
    from .score import lpaps
    cosine = torch.nn.functional.cosine_similarity
    src_stages = None
    if source is not None:
        w, sr = utils.read_wav_channels(source)
        src_stages = [s.float().cpu() for s in scorer.embed_audio([w], sr, stages=True)[1]]
    scores = []
    for k0 in range(0, len(records), batch):
        chunk = records[k0:k0 + batch]
        by_rate = {}
        for k, r in enumerate(chunk):
            w, sr = utils.read_wav_channels(os.path.join(results, r["file"]))
            by_rate.setdefault(sr, []).append((k, w))
        out = [None] * len(chunk)
        text = scorer.embed_text([prompt_of(r) for r in chunk]).float().cpu()
        for sr, items in by_rate.items():           # (one forward pass per sample rate present in the batch)
            rows = [k for k, _ in items]
            emb = scorer.embed_audio([w for _, w in items], sr, stages=src_stages is not None)
            emb, stages = emb if src_stages is not None else (emb, None)
            clap = cosine(emb.float().cpu(), text[rows], dim=1, eps=1e-8).tolist()
            dist = None
            if stages is not None:
                dist = lpaps([s.expand(len(rows), -1, -1) for s in src_stages], [s.float().cpu() for s in stages]).tolist()
            for j, k in enumerate(rows):
                out[k] = dict(index=chunk[k].get("index", k0 + k), file=chunk[k]["file"], clap=clap[j])
                if dist is not None:
                    out[k]["lpaps"] = dist[j]
        scores += out
    ranking = sorted(range(len(scores)), key=lambda k: -scores[k]["clap"])
    return scores, ranking


def write_scores(manifest_path, scores, ranking, header):
    path = os.path.join(os.path.dirname(manifest_path), "scores.json")
    with open(path, "w") as f:
        json.dump(dict(**header, scores=scores, ranking=ranking), f, indent=1)
    return path


def main(argv=None, scorer=None):
    args = parse_args(argv)
    manifest = find_manifest(args.results, args.json)
    records = read_records(manifest)
    if scorer is None:
        from .score import ClapScorer
        scorer = ClapScorer.from_pretrained(args.clap, torch.device(f"cuda:{args.device_num}"), text=args.text_clap,
                                            audio=args.audio_clap)
    towers = scorer.towers
    print(f"CLAP towers: text {towers['text']}, audio {towers['audio']}; resampler: native windowed sinc")
    scores, ranking = score_records(scorer, args.results, records, args.source, args.batch)
    path = write_scores(manifest, scores, ranking, dict(manifest=os.path.basename(manifest), clap=args.clap, source=args.source,
                                                        towers=towers))
    best = scores[ranking[0]]
    print(f"{len(scores)} edits scored -> {path}; best CLAP {best['clap']:.4f} ({best['file']})")


if __name__ == "__main__":
    main()

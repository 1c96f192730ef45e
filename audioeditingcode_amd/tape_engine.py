"""What the text stacks on the op tape (t5.T5EncoderEngine, lm.GPT2Engine and their wrappers) have in common: reading a
checkpoint and its config, packing weights, a small LRU of per-shape plans (tape + buffers + one captured hipGraph each) and the
run of a plan on the engine's side stream."""
import collections
import json
import os
from types import SimpleNamespace

import torch

from . import _lib as L
from . import tape as tape_mod


def config_dict(config, defaults, int_keys):
    """The fields of `defaults`, from a transformers config, any object with those attributes, or a dict (config.json); a
    missing or None field takes its default, the `int_keys` are cast."""
    get = config.get if isinstance(config, dict) else lambda k, d=None: getattr(config, k, d)
    out = {k: (get(k, d) if get(k, d) is not None else d) for k, d in defaults.items()}
    for k in int_keys:
        out[k] = int(out[k])
    return out


def read_checkpoint(path):
    """(config dict, state dict on the host) of a checkpoint directory: config.json + model.safetensors | sharded safetensors |
    pytorch_model.bin, without building a torch module."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    sd = {}
    index = os.path.join(path, "model.safetensors.index.json")
    single = os.path.join(path, "model.safetensors")
    if os.path.exists(single) or os.path.exists(index):
        from safetensors.torch import load_file
        files = [single]
        if not os.path.exists(single):
            with open(index) as f:
                files = sorted({os.path.join(path, v) for v in json.load(f)["weight_map"].values()})
        for fn in files:
            sd.update(load_file(fn))
    elif os.path.exists(os.path.join(path, "pytorch_model.bin")):
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{path}: no model.safetensors, model.safetensors.index.json or pytorch_model.bin")
    return {k: v for k, v in cfg.items() if not k.startswith("_")}, sd


class TapeEngine:
    """Base of an engine that packs a state dict into `self.w` and builds one plan per input shape with `build_plan(*shape)`:
    a dict that holds the plan's `tape` and a `graph` flag (False until the tape is captured)."""

    MAX_SHAPES = 4              # plans kept (tape + activations + one instantiated hipGraph each; weights are shared)

    def __init__(self, device):
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self._plans = collections.OrderedDict()

    # ------------------------------------------------------------------ weights
    def _get(self, sd, *names):
        """The first of `names` the state dict has, as fp32."""
        for n in names:
            if n in sd:
                return sd[n].detach().to(torch.float32)
        raise L.AedError(f"{type(self).__name__}: the state dict has no '{names[0]}'")

    def _put(self, t, shape):
        if tuple(t.shape) != tuple(shape):
            raise L.AedError(f"{type(self).__name__}: a weight has shape {tuple(t.shape)}, the config says {tuple(shape)}")
        return t.contiguous().to(self.device)

    @property
    def weight_bytes(self):
        """Device memory of the packed weights."""
        return sum(t.numel() * t.element_size() for t in self.w.values())

    # ------------------------------------------------------------------ plans
    def _plan(self, *shape):
        key = (*shape, getattr(tape_mod._regime, "arith", None) or tape_mod.DEFAULT_ARITH)
        plan = self._plans.pop(key, None)
        if plan is None:
            while len(self._plans) >= self.MAX_SHAPES:
                if self.stream is not None:
                    torch.cuda.synchronize(self.device)         # an evicted plan's graph may still be in flight
                self._plans.popitem(last=False)                 # (its Tape destroys the graph)
            plan = self.build_plan(*shape)
        self._plans[key] = plan                                 # most recently used last
        return plan

    def _require_gpu(self):
        if self.device.type != "cuda":
            raise L.AedError(f"{type(self).__name__} on device={self.device} builds tapes only; running needs an MI355X (HIP) -- "
                             f"there is no CPU fallback")

    def _run(self, plan, fill, use_graph):
        """`fill(plan)` copies the inputs into the plan's buffers and the tape runs, both on the engine's stream, ordered
        after the caller's stream and before what the caller issues next.  With `use_graph` the tape is captured on first
        use and replayed."""
        tp = plan["tape"]
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            fill(plan)
            if not use_graph:
                tp.run()
            else:
                if not plan["graph"]:
                    tp.run()                                    # once outside capture: a refused record raises here
                    tp.capture()
                    plan["graph"] = True
                tp.replay()
        cur.wait_stream(self.stream)


class NativeTextModule:
    """Base of the drop-ins for a transformers module slot of `text_encoders.TextEncoders`: an engine (class `ENGINE`) plus a
    `config` namespace with `model_type` = `MODEL_TYPE`."""

    ENGINE = None
    MODEL_TYPE = None

    def __init__(self, engine, config=None):
        self.engine = engine
        if config is None or isinstance(config, dict):
            config = SimpleNamespace(**{"model_type": self.MODEL_TYPE, **(config or engine.cfg)})
        self.config = config

    @classmethod
    def from_module(cls, hf_module, device):
        """From a live transformers module (its state dict is copied; the module itself is not kept)."""
        return cls(cls.ENGINE(hf_module.config, hf_module.state_dict(), device), hf_module.config)

    @classmethod
    def from_pretrained(cls, path, device):
        """From a checkpoint directory (config.json + model.safetensors | sharded safetensors | pytorch_model.bin) without
        building a torch module."""
        cfg, sd = read_checkpoint(path)
        cfg.setdefault("model_type", cls.MODEL_TYPE)
        return cls(cls.ENGINE(cfg, sd, device), SimpleNamespace(**cfg))

    def parameters(self):
        return iter(self.engine.w.values())

    def eval(self):
        return self

"""LoRA adapters on the decoder layers' fused projections.

    y = x W^T + (alpha / r) (x A^T) B^T        A [r, in] ~ U(-1/sqrt(in), 1/sqrt(in)),  B [out, r] = 0

`apply_lora` freezes every existing parameter and attaches one `LoRAAdapter` per chosen
projection of every `DecoderLayer`: `qkv` (the fused q|k|v projection: per-matrix adapters with
a shared A are a special case of it), `o`, `up` (the fused gate|up projection) and `down`. The
call sites in models/transformer.py route through `ops.lora.lora_linear` while an adapter is
attached and enabled; `lora_disabled(model)` switches them off for a block, which is how DPO
gets its frozen reference from the policy itself (`LoRAReference`). `merge_lora` folds
W += (alpha / r) B A into the base weights and removes the adapters.
"""
from __future__ import annotations

import contextlib
import hashlib
import math
from typing import Dict, Iterable, List, Optional, Tuple

import torch
import torch.nn as nn

from ..ops import lora as lora_ops

TARGETS = ("qkv", "o", "up", "down")
MAX_RANK = 256
# target -> (owning submodule of a DecoderLayer, weight attribute, adapter attribute)
_SITES = {"qkv": ("attn", "qkv_proj", "lora_qkv"), "o": ("attn", "o_proj", "lora_o"),
          "up": ("mlp", "up_proj", "lora_up"), "down": ("mlp", "down_proj", "lora_down")}
CONFIG_KEYS = {"enabled": False, "r": 16, "alpha": 32, "dropout": 0.0, "target_modules": list(TARGETS),
               "save_merged": True}


def lora_config(model_cfg: Optional[dict]) -> dict:
    """The validated `model.lora` block with defaults filled in (ValueError on unknown keys or
    bad values). A missing block is the disabled default."""
    raw = (model_cfg or {}).get("lora") or {}
    if not isinstance(raw, dict):
        raise ValueError(f"model.lora must be a mapping, got {type(raw).__name__}")
    unknown = sorted(set(raw) - set(CONFIG_KEYS))
    if unknown:
        raise ValueError(f"model.lora: unknown key(s) {unknown}; known: {sorted(CONFIG_KEYS)}")
    cfg = {k: (list(v) if isinstance(v, list) else v) for k, v in CONFIG_KEYS.items()}
    cfg.update(raw)
    for k in ("enabled", "save_merged"):
        if not isinstance(cfg[k], bool):
            raise ValueError(f"model.lora.{k} must be true or false, got {cfg[k]!r}")
    _check_hparams(cfg["r"], cfg["alpha"], cfg["dropout"], cfg["target_modules"])
    cfg["target_modules"] = list(cfg["target_modules"])
    return cfg


def _check_hparams(r, alpha, dropout, targets) -> None:
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= MAX_RANK:
        raise ValueError(f"lora r must be an integer in [1, {MAX_RANK}], got {r!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not alpha > 0 or not math.isfinite(alpha):
        raise ValueError(f"lora alpha must be a positive number, got {alpha!r}")
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)) or not 0.0 <= dropout < 1.0:
        raise ValueError(f"lora dropout must be in [0, 1), got {dropout!r}")
    if isinstance(targets, str) or not isinstance(targets, (list, tuple)) or not targets:
        raise ValueError(f"lora target_modules must be a non-empty list out of {list(TARGETS)}, got {targets!r}")
    bad = [t for t in targets if t not in TARGETS]
    if bad or len(set(targets)) != len(targets):
        raise ValueError(f"lora target_modules must be distinct names out of {list(TARGETS)}, got {list(targets)!r}")


def _adapter_seed(seed: int, name: str) -> int:
    h = hashlib.sha256(f"{int(seed)}:{name}".encode()).digest()
    return int.from_bytes(h[:8], "little") % (2 ** 62)


class LoRAAdapter(nn.Module):
    """A [r, in], B [out, r] of one projection. The values depend on (seed, qualified name) only:
    every rank draws the same ones and the attach order does not matter."""

    def __init__(self, in_features: int, out_features: int, r: int, alpha: float, dropout: float,
                 seed: int, name: str, device=None, dtype=None):
        super().__init__()
        self.r, self.alpha, self.dropout = int(r), float(alpha), float(dropout)
        self.scale = float(alpha) / int(r)
        self.enabled = True
        self.qualified_name = name
        gen = torch.Generator(device="cpu")
        gen.manual_seed(_adapter_seed(seed, name))
        bound = 1.0 / math.sqrt(in_features)
        a = (torch.rand((r, in_features), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
        self.A = nn.Parameter(a.to(device=device, dtype=dtype))
        self.B = nn.Parameter(torch.zeros((out_features, r), device=device, dtype=dtype))

    def forward(self, x, weight, bias=None, resid=None):
        return lora_ops.lora_linear(x, weight, self.A, self.B, self.scale, bias=bias, resid=resid,
                                    dropout=self.dropout, training=self.training)

    def delta(self) -> torch.Tensor:
        """scale * B A in fp32."""
        return self.scale * (self.B.detach().float() @ self.A.detach().float())

    def extra_repr(self) -> str:
        return f"r={self.r}, alpha={self.alpha}, dropout={self.dropout}, enabled={self.enabled}"


def _causal_lm(model):
    """The CausalLM inside `model` (a CausalLM, or a reward / value model around a backbone)."""
    return getattr(model, "backbone", model)


def lora_sites(model) -> Iterable[Tuple[str, nn.Module, str, str]]:
    """(qualified adapter name, owning module, weight attribute, adapter attribute) of every
    attached adapter, in layer order."""
    lm = _causal_lm(model)
    prefix = "backbone." if lm is not model else ""
    for i, layer in enumerate(getattr(lm, "layers", [])):
        for t in TARGETS:
            sub, wname, aname = _SITES[t]
            owner = getattr(layer, sub, None)
            if owner is not None and getattr(owner, aname, None) is not None:
                yield f"{prefix}layers.{i}.{sub}.{aname}", owner, wname, aname


def lora_adapters(model) -> List[LoRAAdapter]:
    return [getattr(owner, aname) for _, owner, _, aname in lora_sites(model)]


def has_lora(model) -> bool:
    return next(iter(lora_sites(model)), None) is not None


def has_active_lora(model) -> bool:
    return any(a.enabled for a in lora_adapters(model))


def _refuse_unsupported(lm) -> None:
    cfg = lm.cfg
    if cfg.is_moe:
        raise ValueError("LoRA is not supported on MoE layers")
    if getattr(lm, "tp", None) is not None or getattr(lm, "tp_size", 1) > 1 or getattr(lm, "tp_seq", None) is not None:
        raise ValueError("LoRA is not supported with tensor parallelism")
    if getattr(lm, "sp", None) is not None:
        raise ValueError("LoRA is not supported with sequence parallelism")
    if getattr(lm, "ep_size", 1) > 1:
        raise ValueError("LoRA is not supported with expert parallelism")
    if getattr(lm, "layer_devices", None) is not None:
        raise ValueError("LoRA is not supported with layer_split")
    if lm.sharding_engines():
        raise ValueError("LoRA is not supported with ZeRO-3 / FSDP (use data parallel or ZeRO-1)")
    for layer in lm.layers:
        if getattr(layer.attn, "tp", None) is not None or getattr(layer.mlp, "tp", None) is not None \
                or getattr(layer.attn, "sp", None) is not None:
            raise ValueError("LoRA is not supported with tensor or sequence parallelism")


def apply_lora(model, r: int = 16, alpha: float = 32, dropout: float = 0.0,
               target_modules=TARGETS, seed: int = 0, save_merged: bool = True,
               base_model: Optional[str] = None) -> Dict[str, float]:
    """Freeze every existing parameter of `model` and attach adapters to the chosen projections of
    every decoder layer. Call it after the base is built / loaded / materialised and
    parallelised, before the training engine is made. Base tensors are not touched.
    `save_merged` / `base_model` are recorded for the checkpoint writer (utils/checkpoint.py).
    Returns `count_trainable_params(model)`."""
    _check_hparams(r, alpha, dropout, list(target_modules) if not isinstance(target_modules, str) else target_modules)
    lm = _causal_lm(model)
    if not hasattr(lm, "layers") or not hasattr(lm, "cfg"):
        raise ValueError(f"apply_lora needs a CausalLM (or a model around one), got {type(model).__name__}")
    _refuse_unsupported(lm)
    if has_lora(model):
        raise ValueError("the model already has LoRA adapters (merge_lora first)")
    if any(p.is_meta for p in lm.parameters()):
        raise ValueError("apply_lora runs after the base weights are materialised")
    prev = {id(p): p.requires_grad for p in model.parameters()}
    for p in lm.parameters():
        p.requires_grad_(False)
    lm._dla_lora_prev_requires_grad = prev
    prefix = "backbone." if lm is not model else ""
    for i, layer in enumerate(lm.layers):
        for t in target_modules:
            sub, wname, aname = _SITES[t]
            owner = getattr(layer, sub)
            w = getattr(owner, wname)
            name = f"{prefix}layers.{i}.{sub}.{aname}"
            setattr(owner, aname, LoRAAdapter(w.shape[1], w.shape[0], r, alpha, dropout, seed, name,
                                              device=w.device, dtype=w.dtype))
    lm._dla_lora = {"r": int(r), "alpha": float(alpha), "dropout": float(dropout),
                    "target_modules": list(target_modules), "save_merged": bool(save_merged),
                    "base_model_name_or_path": None if base_model is None else str(base_model)}
    from .loader import count_trainable_params

    return count_trainable_params(model)


@contextlib.contextmanager
def lora_disabled(model):
    """Inside the block the adapter call sites run the base path (same kernels and bits as a model
    without adapters)."""
    ads = lora_adapters(model)
    prev = [a.enabled for a in ads]
    for a in ads:
        a.enabled = False
    try:
        yield model
    finally:
        for a, e in zip(ads, prev):
            a.enabled = e


class LoRAReference:
    """The frozen reference of an adapter policy: the same model with its adapters switched off
    and no autograd. Attribute access is delegated; the forward entry points the objectives use
    run under `lora_disabled` and `no_grad`. `RefLogpsStream` and `dpo_step_loss` take it in
    place of a second model."""

    _WRAPPED = ("sequence_logprob", "token_logprobs", "_masked_token_logprob")

    def __init__(self, model):
        if not has_lora(model):
            raise ValueError("LoRAReference needs a model with LoRA adapters attached")
        self.__dict__["_model"] = model

    def _off(self, fn, *args, **kwargs):
        with lora_disabled(self._model), torch.no_grad():
            return fn(*args, **kwargs)

    def __call__(self, *args, **kwargs):
        return self._off(self._model, *args, **kwargs)

    def __getattr__(self, name):
        attr = getattr(self.__dict__["_model"], name)
        if name in LoRAReference._WRAPPED:
            return lambda *a, **k: self._off(attr, *a, **k)
        return attr

    def __setattr__(self, name, value):
        setattr(self.__dict__["_model"], name, value)


@torch.no_grad()
def merged_weight(weight: torch.Tensor, adapter: LoRAAdapter) -> torch.Tensor:
    """W + scale * B A as a new tensor: the product and the sum in fp32, rounded once."""
    return (weight.detach().float() + adapter.delta().to(weight.device)).to(weight.dtype)


@torch.no_grad()
def merge_lora(model):
    """Fold W += scale * B A into the base weights in place (fp32 product, one rounding), remove
    the adapters and restore the parameters' `requires_grad`."""
    lm = _causal_lm(model)
    for _, owner, wname, aname in list(lora_sites(model)):
        w = getattr(owner, wname)
        w.copy_(merged_weight(w, getattr(owner, aname)))
        setattr(owner, aname, None)
    prev = lm.__dict__.pop("_dla_lora_prev_requires_grad", None)
    for p in model.parameters():
        p.requires_grad_(prev.get(id(p), True) if prev is not None else True)
    lm.__dict__.pop("_dla_lora", None)
    return model


def adapter_state_dict(model) -> Dict[str, torch.Tensor]:
    """Everything an adapter model trains, under module names: A and B of every adapter
    (`layers.3.attn.lora_qkv.A` ...) and every other parameter left trainable outside the frozen
    base (the reward model's score head, `scorer.1.weight` / `scorer.1.bias`)."""
    out = {}
    for name, owner, _, aname in lora_sites(model):
        ad = getattr(owner, aname)
        out[f"{name}.A"] = ad.A.detach()
        out[f"{name}.B"] = ad.B.detach()
    for name, p in model.named_parameters():
        if p.requires_grad and name not in out:
            out[name] = p.detach()
    return out


@torch.no_grad()
def load_adapter_state_dict(model, sd: Dict[str, torch.Tensor]) -> None:
    want = adapter_state_dict(model)
    missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or extra:
        raise ValueError(f"adapter file does not match the model: missing {missing[:4]}, unexpected {extra[:4]}")
    for k, dst in want.items():
        if tuple(sd[k].shape) != tuple(dst.shape):
            raise ValueError(f"adapter tensor {k}: shape {tuple(sd[k].shape)} vs {tuple(dst.shape)}")
        dst.copy_(sd[k].to(device=dst.device, dtype=dst.dtype))


def merged_overrides(model) -> Dict[int, torch.Tensor]:
    """id(base weight) -> adapter, for writers that merge per tensor while streaming."""
    return {id(getattr(owner, wname)): getattr(owner, aname) for _, owner, wname, aname in lora_sites(model)}

"""What every wrapper module needs around a call into libboxinst_hip.so: the current stream's handle, the device check of the
tensor arguments, a tensor's address, and access to a config block that is a dict or a namespace."""
from __future__ import annotations

import torch

_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def current_stream(dev: torch.device) -> int:
    """The current stream's handle (the raw getter skips building a Stream object: 0.3 instead of 1.9 us)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


def need_cuda(**tensors) -> None:
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError(f'{name} must be a CUDA (HIP) tensor: boxinstseg_amd has no CPU path')


def ptr(t):
    return None if t is None else t.data_ptr()


def cfg_get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


def cfg_require(cfg, name):
    """As cfg_get, but a missing key raises: KeyError for a dict, AttributeError for a namespace."""
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def cfg_keys(cfg):
    return list(cfg.keys()) if isinstance(cfg, dict) else [k for k in vars(cfg) if not k.startswith('_')]


def cfg_only(cfg, where, allowed):
    for k in cfg_keys(cfg):
        if k not in allowed:
            raise NotImplementedError(f'{where}.{k} is not supported')

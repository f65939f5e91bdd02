"""Shared by the engine's and the renderer's modules (imports nothing from the package): tensor conversions, the device decorator."""
import functools

import torch


def f32(t: torch.Tensor) -> torch.Tensor:
    """``t`` as the library reads it: detached, fp32, contiguous (no copy when it already is fp32 and contiguous)."""
    return t.detach().to(torch.float32).contiguous()


def u8(valid: torch.Tensor) -> torch.Tensor:
    """A per-ray validity mask as the bytes the library reads (a bool tensor is reinterpreted, not converted)."""
    return (valid.view(torch.uint8) if valid.dtype == torch.bool else valid.to(torch.uint8)).contiguous()


def _on_device(fn):
    """Run a public renderer method with the renderer's GPU as the current HIP device (the C ABI launches on the current
    device), so that several renderers on different GPUs can live in one process."""
    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        if torch.cuda.current_device() == self.device.index:
            return fn(self, *a, **k)
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapped


def mixed_in(mixin):
    """Class decorator: the methods of ``mixin`` become methods of the decorated class, which keeps its list of base classes (the
    chains of ``Engine`` and of the renderer are three and two classes long, and tests/test_module_split_host.py holds them to that).
    A name that the class or one of its bases already defines is refused, so nothing is shadowed silently."""
    def apply(cls):
        for name, value in vars(mixin).items():
            if name.startswith("__") and name.endswith("__"):
                continue
            for c in cls.__mro__:
                if c is not object and name in vars(c):
                    raise TypeError(f"{name} is defined in {c.__name__} and in {mixin.__name__}")
            setattr(cls, name, value)
        return cls
    return apply

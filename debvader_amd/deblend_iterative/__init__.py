"""Iterative deblending of a field (reference: src/debvader/deblend_iterative/).

IterativeDeblendField is the reference's class; IterativeDeblendFieldBatch runs its loop for many fields that stay on the
GPU.  Both resolve on first use, like the names of the package root: importing the sub-package
alone loads neither pandas nor the HIP library.
"""
_LAZY = ("IterativeDeblendField", "IterativeDeblendFieldBatch")

__all__ = list(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib

        value = getattr(importlib.import_module("debvader_amd.deblend_iterative.iterative_deblender"), name)
        globals()[name] = value
        return value
    raise AttributeError(f"module 'debvader_amd.deblend_iterative' has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_LAZY))

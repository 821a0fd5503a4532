"""The Python layer's switches, resolved once.

`Settings` lists everything that can be switched above the C library; `current()` is the instance in force.  The environment
is read ONCE, when this module is imported (`Settings.from_env`); afterwards a value changes only through `replace` /
`override` (or the named setters built on them: `fused.set_conv_precision`, `fused.set_fusion`, `modules.set_me_conv`,
`modules.set_me_norm`).  A write to `os.environ` after the import has no effect.

Process-wide means what `os.environ` meant: there is one instance and ALL threads see it.  `override` is for tests and
tools that A/B a switch, not for scenes in flight on several threads - per-thread run state of a step (`fused.precision_override`,
`fused.optimistic_override`) stays thread-local in `pasco_amd.graph.fused`.

Imports nothing of `pasco_amd` and not torch: every module of the package can import it."""
from __future__ import annotations

import contextlib
import dataclasses
import os
from typing import Mapping


@dataclasses.dataclass(frozen=True)
class Settings:
    # bool, on unless the variable is exactly "0"
    query_graph: bool = True       # PASCO_QUERY_GRAPH      query-side transformer ops replayed from captured hipGraphs
    mask_block: bool = True        # PASCO_MASK_BLOCK       block lookups of the attention masks
    pe_table: bool = True          # PASCO_PE_TABLE         table form of the position encoding
    head_absorb: bool = True       # PASCO_HEAD_ABSORB      mask heads absorb the voxel-feature projection
    attn_feat: bool = True         # PASCO_ATTN_FEAT        finest level's attention on the feature operand
    attn_split: bool = True        # PASCO_ATTN_SPLIT       K / V as split operands
    keep_fused: bool = True        # PASCO_KEEP_FUSED       decoder keep masks by the keep_mask kernel
    resize_absorb: bool = True     # PASCO_RESIZE_ABSORB    decoder `resize` without the concatenated tensor
    input_fused: bool = True       # PASCO_INPUT_FUSED      input stage as one fused stage
    optimistic: bool = True        # PASCO_OPTIMISTIC       PascoNet.forward's end-of-step-validated shortcuts
    panoptic_kernel: bool = True   # PASCO_PANOPTIC_KERNEL  panoptic_inference on the device kernels
    conv_rl: bool = True           # PASCO_CONV_RL          row lists of the generative transposed convolutions
    bench_pin: bool = True         # PASCO_BENCH_PIN        dist.pin_rank pins a rank to its GPU's cores
    me_defer: bool = True          # PASCO_ME_DEFER         eval-mode BatchNorm / ReLU recorded, applied by the next convolution
    # bool, on only if the variable is exactly "2"
    conv_win_wide: bool = False    # PASCO_CONV_WIN         window tables for 128-wide layers too (experiments)
    # strings
    c4_exchange: str = "slab"      # PASCO_C4_EXCHANGE      "f16": subnet_parallel_forward ships the mask logits as f16
    me_conv: str = "guarded"       # PASCO_ME_CONV          "guarded" | "exact"
    me_norm: str = "torch"         # PASCO_ME_NORM          "torch" | "device"
    # no environment name
    conv_precision: str = "f16x3"  # "f16x3" | "f32" (fused.set_conv_precision)
    presplit: bool = True          # f16x3 operands pre-split once per tensor (mma_mode 2) instead of per gather (mode 1)
    fusion: bool = True            # False: route (a) of INTEGRATION.md - every block as the reference's own module sequence

    def __post_init__(self):
        assert self.me_conv in ("guarded", "exact"), f"PASCO_ME_CONV={self.me_conv!r}: 'guarded' or 'exact'"
        assert self.me_norm in ("torch", "device"), f"PASCO_ME_NORM={self.me_norm!r}: 'torch' or 'device'"
        assert self.conv_precision in ("f32", "f16x3")

    @classmethod
    def from_env(cls, mapping: Mapping[str, str] = os.environ) -> "Settings":
        """The one place of the package that reads a PASCO_* name."""
        names, env = [f.name for f in dataclasses.fields(cls)], lambda f: "PASCO_" + f.upper()
        got = {f: mapping.get(env(f), "1") != "0" for f in names[:names.index("conv_win_wide")]}
        got.update({f: mapping[env(f)] for f in ("c4_exchange", "me_conv", "me_norm") if env(f) in mapping})
        return cls(conv_win_wide=mapping.get("PASCO_CONV_WIN") == "2", **got)


_current = Settings.from_env()


def current() -> Settings:
    return _current


def replace(**fields) -> Settings:
    """Install a changed copy (TypeError for an unknown field) -> the instance that was in force before."""
    global _current
    prev, _current = _current, dataclasses.replace(_current, **fields)
    return prev


@contextlib.contextmanager
def override(**fields):
    """`replace` for the enclosed block; the previous instance is back afterwards, also after an exception."""
    global _current
    prev = replace(**fields)
    try:
        yield _current
    finally:
        _current = prev

"""C-ABI surface: both shared libraries export every entry point include/pasco_hip.h declares, the
ctypes mirror of `ph_conv_desc` has the C layout, and the product has no CPU path.  No compute."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pasco_hip.h")


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"PH_FN\((\w+)\)\s*\(", src)))


def test_header_declares_expected_entry_points():
    names = declared()
    for must in ("map_insert", "nbr_build", "kmap_compact", "conv_fwd", "maxpool_fwd", "mask_compact",
                 "to_dense", "to_sparse_coords", "attn_cross_fwd", "attn_cross_split"):
        assert must in names


def test_hip_library_exports_every_symbol():
    from pasco_amd.build import build_hip
    lib = ctypes.CDLL(build_hip(verbose=False))
    for n in declared():
        assert hasattr(lib, "ph_" + n), f"libpascohip.so lacks ph_{n}"
    lib.ph_abi_version.restype = ctypes.c_int
    from pasco_amd.me.backend import ABI_VERSION
    assert lib.ph_abi_version() == ABI_VERSION == 5
    from pasco_amd.me.backend import ConvDesc
    assert lib.ph_conv_desc_size() == ctypes.sizeof(ConvDesc)


def _dynamic_exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW"}


def test_product_library_exports_exactly_the_header(tmp_path):
    """No development surface in the product: the `ph_*` symbols libpascohip.so exports are EXACTLY the entry points
    include/pasco_hip.h declares (round 5 shipped 8 undeclared ones: ablation masks, traces, process-global kernel
    forcing), its sources read no environment variable, and the experiment state is compiled only with -DPH_DEV."""
    from pasco_amd.build import CSRC, build_hip
    exported = {s for s in _dynamic_exports(build_hip(verbose=False)) if s.startswith("ph_")}
    assert exported == {"ph_" + n for n in declared()}, sorted(exported ^ {"ph_" + n for n in declared()})
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(CSRC, f)).read()
            body = src.split("#ifdef PH_DEV")[0] if f == "ph_common.h" else src
            assert "getenv(" not in body.replace("PH_DEV_ENV(", ""), f"{f} reads the environment outside the development build"
    # a.ablate is only ever read through PH_ABLATE (the constant 0 in the product build)
    for f in ("conv_dma.hip", "conv_win.hip", "conv_wide.hip", "conv_lin.hip", "conv_f16x3.hip", "conv_h2_common.h"):
        src = open(os.path.join(CSRC, f)).read()
        product = re.sub(r"#ifdef PH_DEV.*?#(?:else|endif)", "", src, flags=re.S)
        assert not re.search(r"\ba\.ablate\s*&", product), f"{f}: ablation branch outside PH_ABLATE"


def test_binding_rejects_other_abi_versions(monkeypatch):
    """A stale library (other PH_ABI_VERSION or another ph_conv_desc size) is refused with a 'rebuild' message instead of
    being called with misaligned arguments."""
    from pasco_amd.build import build_hip
    from pasco_amd.me import backend
    monkeypatch.setattr(backend, "ABI_VERSION", backend.ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        backend.CBackend(build_hip(verbose=False), "ph_", "cuda")


def test_oracle_exports_every_symbol(oracle):
    for n in declared():
        assert hasattr(oracle.lib, "pho_" + n), f"oracle lacks pho_{n}"


def test_conv_desc_layout_matches_c():
    from pasco_amd.me.backend import ConvDesc
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pasco_hip.h"\nint main(){printf("%zu %zu %zu %zu", ' \
           'sizeof(ph_conv_desc), offsetof(ph_conv_desc, cin), offsetof(ph_conv_desc, residual), ' \
           'offsetof(ph_conv_desc, epi2_scale)); return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, o_cin, o_res, o_e2 = [int(v) for v in subprocess.check_output([exe]).split()]
    assert ctypes.sizeof(ConvDesc) == size
    assert ConvDesc.cin.offset == o_cin and ConvDesc.residual.offset == o_res and ConvDesc.epi2_scale.offset == o_e2


def test_no_cpu_path_in_product():
    from pasco_amd.me import backend
    backend.register_checker_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        backend.backend_for(torch.device("cpu"))
    import pasco_amd.me as ME
    with pytest.raises(RuntimeError):
        ME.SparseTensor(torch.zeros(2, 3), torch.zeros(2, 4, dtype=torch.int32))


def test_release_stream_drops_the_per_stream_buffers(oracle):
    """`CBackend.release_stream`: workspaces and the status pair are keyed by (device, raw stream handle); retiring a
    stream drops them, so a recycled handle starts with a clean status word."""
    import torch
    dev = torch.device("cpu")
    oracle.workspace(1000, dev)
    oracle.status_word(dev).fill_(1)
    assert {"status", "ws"} <= oracle.scratch.held()
    assert oracle.release_stream(0) >= 2
    assert not {"status", "ws"} & oracle.scratch.held()
    assert int(oracle.status_word(dev)) == 0          # a fresh pair

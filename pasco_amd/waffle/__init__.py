"""WaffleIron point features (include/pasco_waffle.h): what the scoring commands read from
`waffleiron_v2/sequences/<seq>/seg_feats_tta/<frame>.pkl`, computed from the scan itself.  `host` restates every kernel and
the network, `lib` binds the `pw_*` entry points, `prep` turns one vote of a scan into the network's inputs, `net` is the
network on the kernels, `Extractor` runs the votes of a frame on either and `python -m pasco_amd.waffle` writes the files."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import host, prep  # noqa: F401
from .net import WaffleNet  # noqa: F401


class Extractor:
    """`frame(scan, frame_number)` -> the three arrays of the reference's pickle for one scan."""

    def __init__(self, ckpt: str, config, device="cuda", num_votes: int = 1, seed: int = 0, half: bool = False):
        self.cfg = prep.load_config(config) if isinstance(config, str) else prep.settings(config)
        self.device = torch.device(device)
        self.net = WaffleNet.load(ckpt, self.cfg["grids"], self.device)
        if self.net.cin != sum(3 if name == "xyz" else 1 for name in self.cfg["input_feat"]):
            raise ValueError(f"the checkpoint takes {self.net.cin} input features, the config lists {self.cfg['input_feat']}")
        self.num_votes, self.seed, self.half = int(num_votes), int(seed), bool(half)

    def vote(self, pc: np.ndarray):
        """One prepared cloud -> (embedding [P, C], probabilities [P, classes]) on `self.device`, gathered through upsample."""
        if self.device.type == "cuda":
            it = prep.prepare_device(pc, self.cfg, self.device)
            emb, _, logits = self.net.forward(it["feat"], it["cells"], it["knn"])
            up = it["upsample"].long()
        else:
            it = prep.prepare_host(pc, self.cfg)
            cells = [(torch.from_numpy(c.astype(np.int64)), shape) for c, _, _, shape in it["cells"]]
            with torch.no_grad():
                emb, _, logits = host.forward(self.net, torch.from_numpy(it["feat"]), cells,
                                              torch.from_numpy(it["knn"].astype(np.int64)))
            up = torch.from_numpy(it["upsample"].astype(np.int64))
        return emb[up], torch.softmax(logits[up], dim=1)

    def frame(self, scan: np.ndarray, frame: int = 0) -> Dict[str, np.ndarray]:
        """scan float32 [P, 4] -> {"embedding" [V, C, P], "coords" [P, 4], "vote" [P, classes]}."""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        pc0 = prep.input_features(scan, self.cfg["input_feat"])
        embs, total = [], None
        for v in range(self.num_votes):
            pc = prep.augment(pc0, prep.tta_params(self.seed, frame, v) if self.num_votes > 1 else None)
            emb, prob = self.vote(pc)
            embs.append(emb.t())
            total = prob if total is None else total + prob
        emb = torch.stack(embs, dim=0)
        if self.half:
            emb = emb.half()
        return {"embedding": emb.cpu().numpy(), "coords": pc0[:, :4].copy(), "vote": (total / self.num_votes).cpu().numpy()}

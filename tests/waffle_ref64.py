"""The WaffleIron segmenter written from its definition in plain torch, in any dtype (the reference's own modules cast to
float32 inside, so they cannot run in float64).  One cloud, no padding, channels-first [C, N] as the paper writes it.

    embedding   x = BN(feat);  point = W x + b;  neigh = max_j W2 ReLU(BN(W1 BN(x_j - x_i)));  out = Wf [point; neigh] + bf
    layer       t += s * Inflate(DW(ReLU(DW(Flatten(BN(t))))))     Flatten = per-cell mean with weight 1 / (count + 1e-6)
                t += s * (W2 ReLU(W1 BN(t) + b1) + b2)
    logits      Wc t + bc

`forward(state, grids, feat, cell_ind, neigh, torch.float64)` is the yardstick of the float tests; its float32 twin is held
to the reference's recorded results in tests/test_waffle_cpu.py, which pins this restatement to the reference."""
import torch
import torch.nn.functional as F


def _bn(x, st, prefix, eps=1e-5):
    """x [C, ...]: eval-mode BatchNorm over the leading axis."""
    shape = (-1,) + (1,) * (x.dim() - 1)
    mean, var = st[prefix + ".running_mean"].reshape(shape), st[prefix + ".running_var"].reshape(shape)
    return (x - mean) / torch.sqrt(var + eps) * st[prefix + ".weight"].reshape(shape) + st[prefix + ".bias"].reshape(shape)


def forward(state, grids, feat, cell_ind, neigh, dtype=torch.float64):
    """state: reference key -> array-like; feat [N, F]; cell_ind int [G, N]; neigh int [N, k] (self excluded)
    -> (embedding [N, C], tokens [N, C], logits [N, classes]) in `dtype`."""
    st = {k: torch.as_tensor(v).to(dtype) for k, v in state.items() if "num_batches" not in k}
    x = torch.as_tensor(feat).to(dtype).T                                  # [F, N]
    neigh = torch.as_tensor(neigh).long()
    cell_ind = torch.as_tensor(cell_ind).long()
    N = x.shape[1]
    x = _bn(x, st, "embed.norm")
    point = st["embed.conv1.weight"][:, :, 0] @ x + st["embed.conv1.bias"][:, None]
    rel = x[:, neigh] - x[:, :, None]                                      # [F, N, k]
    rel = _bn(rel, st, "embed.conv2.0")
    rel = torch.einsum("of,fnk->onk", st["embed.conv2.1.weight"][:, :, 0, 0], rel)
    rel = torch.relu(_bn(rel, st, "embed.conv2.2"))
    rel = torch.einsum("oc,cnk->onk", st["embed.conv2.4.weight"][:, :, 0, 0], rel).amax(dim=2)
    emb = st["embed.final.weight"][:, :, 0] @ torch.cat((point, rel), 0) + st["embed.final.bias"][:, None]
    t = emb
    C = t.shape[0]
    depth = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("waffleiron.channel_mix."))
    for d in range(depth):
        g = d % len(grids)
        H, W = grids[g]
        cell = cell_ind[g]
        count = torch.zeros(H * W, dtype=dtype).index_add_(0, cell, torch.ones(N, dtype=dtype))
        p = f"waffleiron.spatial_mix.{d}"
        r = _bn(t, st, p + ".norm") * (1.0 / (count + 1e-6))[cell][None]
        grid = torch.zeros((C, H * W), dtype=dtype).index_add_(1, cell, r).reshape(1, C, H, W)
        grid = F.conv2d(grid, st[p + ".ffn.0.weight"], st[p + ".ffn.0.bias"], padding=1, groups=C)
        grid = F.conv2d(torch.relu(grid), st[p + ".ffn.2.weight"], st[p + ".ffn.2.bias"], padding=1, groups=C)
        t = t + st[p + ".scale.weight"][:, 0, 0][:, None] * grid.reshape(C, H * W)[:, cell]
        p = f"waffleiron.channel_mix.{d}"
        r = _bn(t, st, p + ".norm")
        r = torch.relu(st[p + ".mlp.0.weight"][:, :, 0] @ r + st[p + ".mlp.0.bias"][:, None])
        r = st[p + ".mlp.2.weight"][:, :, 0] @ r + st[p + ".mlp.2.bias"][:, None]
        t = t + st[p + ".scale.weight"][:, 0, 0][:, None] * r
    logits = st["classif.weight"][:, :, 0] @ t + st["classif.bias"][:, None]
    return emb.T.contiguous(), t.T.contiguous(), logits.T.contiguous()

"""Test helper: the cases of the derived-tensor cache tests (tests/test_caches_cpu.py on the CPU oracle, tests/test_hip_caches.py on
the MI355X).  The fused graph keeps tensors derived from the weights on its modules (split kernels, transposed linear weights,
folded BatchNorms, composed projections, captured query graphs: DESIGN.md 4n).  One rule for every case here: after an event
that changes the weights, a WARM net - one that has run and filled its caches - must give what a COLD net gives: a `PascoNet`
constructed now, loaded from the warm net's `state_dict()` and never run before.  The cold net is the only reference, and the
comparison is bit for bit (`bound` = 0.0) where the cold net repeats itself bit for bit.

Every function returns a list of failure lines (empty = passed), each naming the cache entries of the warm net whose tensors
differ from the cold net's."""
import contextlib
import copy

import torch
import torch.nn as nn

from pasco_amd.graph import PascoNet, fused
from pasco_amd.graph.synth import TeacherKeep, make_scene

ROUTES = ("split", "f32", "unfused")
SEEDS = {"A": 3, "B": 4, "C": 5}
_BN = nn.modules.batchnorm._BatchNorm


def build(heavy, device):
    return PascoNet(n_classes=20, n_infers=2, in_channels=16, f=32, num_queries=10, heavy_decoder=heavy).to(device).eval()


def randomise_batchnorms(net, seed):
    """Default BatchNorm state is the same in every net: give each one statistics and an affine map of its own."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, _BN):
                c, dev = m.num_features, m.running_mean.device
                m.running_mean.copy_((torch.randn(c, generator=g) * 0.3).to(dev))
                m.running_var.copy_((torch.rand(c, generator=g) + 0.5).to(dev))
                m.weight.copy_((torch.rand(c, generator=g) + 0.5).to(dev))
                m.bias.copy_((torch.randn(c, generator=g) * 0.1).to(dev))


_CHECKPOINTS = {}


def checkpoint(name, heavy, device):
    """Checkpoint "A" | "B" | "C" as a state dict of fresh tensors (version counter 0, like a loaded file): the caller may hand it
    to `load_state_dict(assign=True)`, which makes its tensors the net's own."""
    key = (name, heavy, str(device))
    if key not in _CHECKPOINTS:
        torch.manual_seed(SEEDS[name])
        net = build(heavy, "cpu")
        randomise_batchnorms(net, SEEDS[name] + 100)
        _CHECKPOINTS[key] = {k: v.detach().to(device) for k, v in net.state_dict().items()}
    return {k: v.clone() for k, v in _CHECKPOINTS[key].items()}


class Bench:
    """The scene, the route and the cold references of one (decoder, route, device)."""

    def __init__(self, heavy, route, device):
        assert route in ROUTES
        self.heavy, self.route, self.device = heavy, route, torch.device(device)
        self.scene = make_scene(4, n_infers=2, in_channels=16, grid=(32, 32, 8), occupancy=0.15).to(self.device)
        self.keep = TeacherKeep(self.scene, self.device)
        self.bound = 0.0          # the GPU leg raises it to 4 x the cold net's own run-to-run difference, if that is not 0
        self._cold = {}

    @contextlib.contextmanager
    def routed(self, route=None):
        route = route or self.route
        with contextlib.ExitStack() as stack:
            if route == "f32":
                stack.enter_context(fused.precision_override("f32"))
            if route == "unfused":
                fused.set_fusion(False)
                stack.callback(fused.set_fusion, True)
            yield

    def run(self, net, mode=torch.no_grad, route=None):
        """One forward (input stage, U-Net, mask transformer) -> the list of output tensors (private copies): the coordinates and
        logits of every subnet at every scale, the voxel and the query logits of the panoptic branch.  The ensembling behind them
        holds no parameter and no entry derived from one; it is left out (it would double the time of a run)."""
        s = self.scene
        with self.routed(route), mode():
            x = net.prepare_input(s.in_feats, s.in_coords)
            ret = net(x, s.global_min_Cs, s.global_max_Cs, s.min_Cs, s.max_Cs, keep_override=self.keep)
            out = []
            for scale in sorted(ret["sem_logits_at_scales"]):
                for t in ret["sem_logits_at_scales"][scale]:
                    out += [t.C, t.F]
            for p in ret["panop_predictions"]:
                out += [p["voxel_logits"].C, p["voxel_logits"].F, p["query_logits"]]
            return [t.detach().clone() for t in out]

    def fresh(self, state):
        net = build(self.heavy, self.device)
        net.load_state_dict(state)
        return net.eval()

    def cold(self, net, route=None):
        """-> (cold net after its one run, its outputs)."""
        c = self.fresh(net.state_dict())
        return c, self.run(c, route=route)

    def cold_of(self, name, route=None):
        """The cold outputs of checkpoint `name`, computed once and shared."""
        key = (name, route or self.route)
        if key not in self._cold:
            self._cold[key] = self.run(self.fresh(checkpoint(name, self.heavy, self.device)), route=route)
        return self._cold[key]

    def warm(self, name="A"):
        net = self.fresh(checkpoint(name, self.heavy, self.device))
        self.run(net)
        return net

    def _graphs_on_this_stream(self, tp):
        """Captured query-side graphs of the current stream (their keys end with the stream's handle)."""
        if self.device.type != "cuda":
            return 0
        handle = torch.cuda.current_stream(self.device).cuda_stream
        return sum(k[-1] == handle for k in tp.__dict__.get("_qgraphs", ()))

    def check(self, what, net, want=None, mode=torch.no_grad, route=None, cold_net=None):
        """Run the warm `net` and compare with `want` (default: a cold net made from its state dict now).  -> failure lines."""
        if want is None:
            cold_net, want = self.cold(net, route=route)
        tp = net.transformer_predictor
        n_graphs = self._graphs_on_this_stream(tp)
        try:
            got = self.run(net, mode=mode, route=route)
        except Exception as exc:          # a failure line per case instead of the first exception
            return [f"{what}: {type(exc).__name__}: {str(exc).splitlines()[0][:160]}"]
        graphs = []
        if self.device.type == "cuda":    # the query side is replayed from captured graphs: still so, and none left behind
            if tp.query_graph_state() != "graph":
                graphs.append(f"{what}: query_graph_state() is {tp.query_graph_state()!r}")
            if n_graphs and self._graphs_on_this_stream(tp) > n_graphs:
                graphs.append(f"{what}: {self._graphs_on_this_stream(tp)} captured graphs of this stream, {n_graphs} before "
                              "the event (a capture under old versions is replaced under its key)")
        d = distance(got, want)
        if d <= self.bound:
            return graphs
        if cold_net is None:              # a cold net that has run, to name the entries that differ from its own
            cold_net = self.cold(net, route=route)[0]
        stale = stale_entries(net, cold_net)
        names = ", ".join(stale[:6]) + (", ..." if len(stale) > 6 else "")
        return graphs + [f"{what}: differs from a cold net by {d:.2e} ({len(stale)} stale entries: {names})"]


def distance(got, want):
    """Largest absolute difference over all outputs; inf where shapes or integer tensors (coordinates) differ."""
    if len(got) != len(want):
        return float("inf")
    d = 0.0
    for a, b in zip(got, want):
        if a.shape != b.shape or a.dtype != b.dtype:
            return float("inf")
        if not a.dtype.is_floating_point:
            if not torch.equal(a, b):
                return float("inf")
        elif a.numel():
            e = float((a.double() - b.double()).abs().max())
            d = max(d, e if e == e else float("inf"))
    return d


# ---- looking into the caches (diagnostics of a failure; the verdict is always the output) --------------------------------------
def _is_cache_name(k):
    return k.startswith(("_ph_", "_roww_", "_split_")) and k != "_ph_source"


def _tensors(v, out):
    if torch.is_tensor(v):
        out.append(v)
    elif isinstance(v, (tuple, list)):
        for e in v:
            _tensors(e, out)
    elif isinstance(v, dict):
        for k in sorted(v, key=str):
            _tensors(v[k], out)
    return out


def cache_entries(net):
    """{"module path._ph_name": [tensors]} of every derived-tensor entry found on the net's modules."""
    found = {}
    for path, m in net.named_modules():
        for k, v in m.__dict__.items():
            if _is_cache_name(k):
                found[f"{path}.{k}"] = _tensors(v, [])
    return found


def stale_entries(warm, cold):
    """Names of the warm net's entries whose tensors are not those of the same entry of the cold net (which has run once)."""
    if cold is None:
        return []
    a, b = cache_entries(warm), cache_entries(cold)
    bad = []
    for name, ts in a.items():
        other = b.get(name)
        if other is None:
            continue          # an entry of a route the cold net did not take
        if len(ts) != len(other) or any(x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x.cpu(), y.cpu())
                                        for x, y in zip(ts, other)):
            bad.append(name)
    return bad


def repeatability(bench):
    """The cold net against itself: two nets from checkpoint A, and one of them run twice.  -> largest difference."""
    a = bench.fresh(checkpoint("A", bench.heavy, bench.device))
    first = bench.run(a)
    d = max(distance(bench.run(a), first), distance(first, bench.cold_of("A")))
    return d


# ---- events ----------------------------------------------------------------------------------------------------------------------
def seeded_sgd_step(net, seed=11, lr=0.05):
    g = torch.Generator().manual_seed(seed)
    params = [p for p in net.parameters()]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(p.device)
    torch.optim.SGD(params, lr=lr).step()
    for p in params:
        p.grad = None


def event_load_in_place(bench):
    """1. load_state_dict(B) into a net warmed with A."""
    net = bench.warm()
    net.load_state_dict(checkpoint("B", bench.heavy, bench.device))
    return bench.check("load_state_dict(B)", net, bench.cold_of("B"))


def event_load_assign(bench):
    """2. load_state_dict(assign=True): B, run, C - every assigned tensor arrives with version counter 0 - and then the tensors of
    another live module, whose counters equal the warm net's own."""
    h, dev = bench.heavy, bench.device
    net = bench.warm()
    net.load_state_dict(checkpoint("B", h, dev), assign=True)
    bad = bench.check("assign B", net, bench.cold_of("B"))
    net.load_state_dict(checkpoint("C", h, dev), assign=True)
    bad += bench.check("assign C", net, bench.cold_of("C"))
    other = bench.fresh(checkpoint("B", h, dev))           # live module: its parameters were copied into once, as the net's were
    net = bench.warm()
    net.load_state_dict(other.state_dict(), assign=True)
    bad += bench.check("assign from a live module", net, bench.cold_of("B"))
    with torch.no_grad():                                  # the two nets now share storage: the live module's update is the net's
        for p in other.parameters():
            p.mul_(1.125)
    bad += bench.check("update through the live module", net)
    return bad


def event_sgd_step(bench):
    """3. one optimiser step with seeded gradients."""
    net = bench.warm()
    seeded_sgd_step(net)
    return bench.check("SGD step", net)


def event_batchnorm_buffers(bench):
    """4. the running statistics alone, rewritten with copy_."""
    net = bench.warm()
    src = checkpoint("B", bench.heavy, bench.device)
    with torch.no_grad():
        for path, m in net.named_modules():
            if isinstance(m, _BN):
                m.running_mean.copy_(src[path + ".running_mean"])
                m.running_var.copy_(src[path + ".running_var"])
    return bench.check("BatchNorm buffers copy_", net)


# tensors whose change must NOT move the output, with the reason; every other (class, name) pair must move it
EXEMPT = {
    ("BatchNorm1d", "num_batches_tracked"): "a step counter: eval-mode normalisation does not read it",
    ("BatchNorm3d", "num_batches_tracked"): "a step counter: eval-mode normalisation does not read it",
}


# tensors that feed an entry kept on ANOTHER module (a sibling, not an ancestor), swept besides the one instance per pair
ELSEWHERE = (
    "transformer_predictor.input_projs.0.weight",          # _ph_composed / _ph_composed_feat of cross-attention layer 0
    "transformer_predictor.input_projs.0.bias",
    "transformer_predictor.mask_feat_proj.bias",
    "transformer_predictor.transformer_cross_attention_layers.0.multihead_attn.out_proj.bias",
    "unet3d.decoder_generative.dec_blocks.0.resize.0.bn.running_var",      # _ph_resize of the decoder block
    "unet3d.decoder_generative.dec_blocks.0.resize.1.bias",
)


def _pairs(net):
    """One instance per (owner class, tensor name) of the WARM net: the first in module order that has a derived entry on itself,
    its parent or its grandparent (where the entries of its tensors live), else the first; then the tensors of ELSEWHERE.
    -> [(class, name, path, module, is_param)]."""
    mods = dict(net.named_modules())

    def near_an_entry(path):
        parts = path.split(".")
        return any(any(_is_cache_name(k) for k in mods[".".join(parts[:n])].__dict__) for n in range(len(parts), max(len(parts) - 3, 0), -1))

    first, best = {}, {}
    for path, m in mods.items():
        own = [(n, True) for n in m._parameters if m._parameters[n] is not None] + \
              [(n, False) for n in m._buffers if m._buffers[n] is not None]
        for name, is_param in own:
            key = (type(m).__name__, name)
            first.setdefault(key, (key[0], name, path, m, is_param))
            if key not in best and near_an_entry(path):
                best[key] = (key[0], name, path, m, is_param)
    out = [best.get(k, v) for k, v in first.items()]
    taken = {f"{p[2]}.{p[1]}" for p in out}
    for full in ELSEWHERE:
        path, name = full.rsplit(".", 1)
        if full not in taken:
            out.append((type(mods[path]).__name__, name, path, mods[path], name in mods[path]._parameters))
    return out


def _perturbed(t, k):
    """Another value of the same kind (variances stay positive, counters stay integers)."""
    if not t.dtype.is_floating_point:
        return t + 1 + k
    return t * (1.25 if k == 0 else 0.75) + (0.0625 if k == 0 else -0.03125) * (t.abs() + 0.25)


def same_counter(value, old):
    """A new tensor holding `value` whose version counter equals `old`'s (an nn.Parameter made of it shares the counter): only
    the object's identity tells it from the tensor it replaces - a key of counters, with or without the device, cannot."""
    new = value.detach().clone()               # counter 0
    while new._version < old._version:
        new.add_(0)
    return new


def event_one_tensor_at_a_time(bench, exempt=EXEMPT):
    """5. for every (owner class, tensor name) pair one instance is changed alone: in place under no_grad, then replaced by a new
    nn.Parameter / buffer object at the SAME version counter (`same_counter`).  The states accumulate; after each change the warm net must equal a cold net made from its state
    dict, and the cold output must have moved unless the pair is exempt.
    -> (failure lines, pairs covered, tensors of ELSEWHERE swept besides, pairs exempt)."""
    net = bench.warm()
    before = bench.cold_of("A")
    bad, covered, exempted = [], 0, 0
    mods = dict(net.named_modules())
    todo = _pairs(net)
    n_pairs = len({(p[0], p[1]) for p in todo})
    for cls, name, path, _, is_param in todo:
        covered += 1
        is_exempt = (cls, name) in exempt
        exempted += is_exempt and covered <= n_pairs
        for k, way in enumerate(("in place", "replaced")):
            mod = mods[path]
            with torch.no_grad():
                t = getattr(mod, name)
                if way == "in place":
                    t.copy_(_perturbed(t, k))
                else:
                    new = same_counter(_perturbed(t, k), t)
                    setattr(mod, name, nn.Parameter(new, requires_grad=t.requires_grad) if is_param else new)
                    assert getattr(mod, name)._version == t._version and getattr(mod, name) is not t
            what = f"{cls}.{name} ({path}) {way}"
            cold_net, want = bench.cold(net)
            moved = distance(want, before) > bench.bound
            if moved and is_exempt:
                bad.append(f"{what}: exempt ({exempt[(cls, name)]}), but the cold output moved")
            if not moved and not is_exempt:
                bad.append(f"{what}: the cold output did not move - the case checks nothing")
            lines = bench.check(what, net, want, cold_net=cold_net)
            if lines:
                bad += lines
                net = cold_net          # carry no stale entry into the next pair: it has run once with exactly this state
                mods = dict(net.named_modules())
            before = want
    return bad, n_pairs, covered - n_pairs, exempted


def event_inference_mode(bench):
    """6. torch.inference_mode(), every run equal to the cold no_grad run of checkpoint A."""
    h, dev, want = bench.heavy, bench.device, bench.cold_of("A")
    net = bench.warm()
    bad = bench.check("warm under no_grad, run under inference_mode", net, want, mode=torch.inference_mode)
    bad += bench.check("... and under no_grad again", net, want)
    net = bench.fresh(checkpoint("A", h, dev))
    bad += bench.check("first run under inference_mode", net, want, mode=torch.inference_mode)
    bad += bench.check("... then under no_grad", net, want)
    try:
        with torch.inference_mode():
            net = bench.fresh(checkpoint("A", h, dev))
    except Exception as exc:
        return bad + [f"constructed under inference_mode: {type(exc).__name__}: {str(exc).splitlines()[0][:160]}"]
    bad += bench.check("constructed and loaded under inference_mode", net, want, mode=torch.inference_mode)
    bad += bench.check("... its second run", net, want, mode=torch.inference_mode)
    return bad


def event_deepcopy(bench):
    """7. copy.deepcopy of a warm net: the copy follows its own weights, the original keeps its own."""
    net = bench.warm()
    try:
        twin = copy.deepcopy(net)
    except Exception as exc:
        return [f"deepcopy of a warm net: {type(exc).__name__}: {str(exc).splitlines()[0][:160]}"]
    bad = bench.check("deep copy, unchanged", twin, bench.cold_of("A"))
    twin.load_state_dict(checkpoint("B", bench.heavy, bench.device))
    bad += bench.check("deep copy loaded with B", twin, bench.cold_of("B"))
    bad += bench.check("the original after its copy diverged", net, bench.cold_of("A"))
    with torch.no_grad():
        for p in twin.parameters():
            p.mul_(0.875)
    bad += bench.check("deep copy updated in place", twin)
    bad += bench.check("the original, again", net, bench.cold_of("A"))
    return bad


def event_round_trips(bench):
    """8. one warm net through the other routes and back: f32 products, the unfused module sequence, and a weight change made
    while the other route's entries are the current ones."""
    assert bench.route == "split"
    net = bench.warm()
    bad = bench.check("precision_override(f32)", net, bench.cold_of("A", "f32"), route="f32")
    bad += bench.check("back on split operands", net, bench.cold_of("A"))
    bad += bench.check("set_fusion(False)", net, bench.cold_of("A", "unfused"), route="unfused")
    bad += bench.check("fused again", net, bench.cold_of("A"))
    net.load_state_dict(checkpoint("B", bench.heavy, bench.device))
    bad += bench.check("B loaded, f32", net, bench.cold_of("B", "f32"), route="f32")
    bad += bench.check("B loaded, unfused", net, bench.cold_of("B", "unfused"), route="unfused")
    bad += bench.check("B loaded, split operands", net, bench.cold_of("B"))
    return bad


def event_freeze(bench):
    """Freezing the parameters (requires_grad_(False)) changes no value and must change no output."""
    net = bench.warm()
    net.requires_grad_(False)
    bad = bench.check("frozen parameters", net, bench.cold_of("A"))
    net.load_state_dict(checkpoint("B", bench.heavy, bench.device))
    return bad + bench.check("frozen parameters, B loaded", net, bench.cold_of("B"))


# ---- device only ---------------------------------------------------------------------------------------------------------------
def event_two_streams(bench):
    """Warm on streams s0 and s1, one after the other; load B on the default stream; run on s1: an entry published by another
    stream and a graph captured under the old versions must both be replaced."""
    dev = bench.device
    want_a, want_b = bench.cold_of("A"), bench.cold_of("B")
    net = bench.fresh(checkpoint("A", bench.heavy, dev))
    torch.cuda.synchronize(dev)
    s0, s1 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    bad = []
    for name, s in (("s0", s0), ("s1", s1)):
        with torch.cuda.stream(s):
            bad += bench.check(f"checkpoint A on stream {name}", net, want_a)
        s.synchronize()
    n_warm = len(net.transformer_predictor.__dict__.get("_qgraphs", ()))
    net.load_state_dict(checkpoint("B", bench.heavy, dev))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s1):
        bad += bench.check("B loaded on the default stream, run on s1", net, want_b)
    s1.synchronize()
    with torch.cuda.stream(s0):
        bad += bench.check("... and on s0", net, want_b)
    s0.synchronize()
    if len(net.transformer_predictor.__dict__.get("_qgraphs", ())) != n_warm:
        bad.append(f"two streams: {len(net.transformer_predictor.__dict__['_qgraphs'])} captured graphs after the load, {n_warm} before")
    from pasco_amd.graph.transformer import release_stream_graphs
    release_stream_graphs(s0), release_stream_graphs(s1)
    return bad


def event_cpu_round_trip(bench):
    """net.cpu() then net.cuda() of a warm net (the storage moves, objects and counters stay): unchanged, then with B loaded."""
    net = bench.warm()
    net.cpu()
    net.to(bench.device)
    bad = bench.check("cpu() then cuda()", net, bench.cold_of("A"))
    net.load_state_dict(checkpoint("B", bench.heavy, bench.device))
    bad += bench.check("cpu() then cuda(), B loaded in place", net, bench.cold_of("B"))
    net.cpu()
    net.load_state_dict(checkpoint("C", bench.heavy, "cpu"))          # changed while away: the counters move on the host
    net.to(bench.device)
    return bad + bench.check("C loaded on the host, then cuda()", net, bench.cold_of("C"))


DEVICE_EVENTS = {"two_streams": event_two_streams, "cpu_round_trip": event_cpu_round_trip}
EVENTS = {"load": event_load_in_place, "assign": event_load_assign, "sgd": event_sgd_step, "bn_buffers": event_batchnorm_buffers,
          "inference_mode": event_inference_mode, "deepcopy": event_deepcopy, "freeze": event_freeze}

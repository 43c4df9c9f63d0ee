"""What the encoders of this package share (`LxmertEncoder` in lxmert.py, `VisualBertModel` in visualbert.py, `ViTModel` in vit.py,
`LayoutLMModel` in layoutlm.py): the draw of the synthetic weights, the parameter spec of a BERT layer, the load of a head wrapper's
state dict, and `BertOps`: the packed weights, the ops over the C ABI, the BERT layer built from them, the rule that picks an
attention entry point, and the front between a caller and `_forward` (check -> forward -> synchronize; capture and replay).  All
arithmetic runs in `libvltk_hip.so`; torch only owns the device buffers.  No CPU fallback.
"""
import zlib

import numpy as np
import torch

from . import _lib as L
from .layers import DTYPES, pack, stream

LN_EPS = 1e-12


def is_gamma(name):
    """Whether a state-dict name is a LayerNorm's weight: spelled out, or the LayerNorm at index 2 of the answer head's nn.Sequential."""
    return "LayerNorm.weight" in name or "layer_norm.weight" in name or name.endswith("logit_fc.2.weight")


def seeded_tensor(name, shape, seed):
    """One tensor of the synthetic state dicts: its own generator, keyed by the seed and the tensor's name."""
    g = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
    if is_gamma(name):
        v = g.uniform(0.5, 1.5, shape)
    else:
        v = g.standard_normal(shape) * 0.05
    return v.astype(np.float32)


def to_numpy(sd):
    return {k: (v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)) for k, v in sd.items()}


def host_array(a):
    """A tensor (read back from its device) or anything array-like -> numpy, for the checks that need an input's values."""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def require_gelu(cfg):
    if cfg["hidden_act"] != "gelu":
        raise NotImplementedError(f"hidden_act '{cfg['hidden_act']}': the GEMM epilogue has the erf GELU only")


def additive_mask(m, device):
    """[B, L] 1 / 0 mask -> the additive `(1 - m) * finfo.min` row the attention kernels take (LxmertModel.forward :766-784)."""
    return None if m is None else ((1.0 - m.to(device, torch.float32)) * torch.finfo(torch.float32).min).contiguous()


def check_text_inputs(input_ids, token_type_ids, cfg):
    """What the embedding kernels trust about the text side: `input_ids [B, Lt]` within the word table, `token_type_ids` (or None)
    of the same shape within the token-type table, `Lt` within the position table.  Host-side (a device tensor is read back), so it
    runs before a launch or a graph capture, never inside one.  A wrong shape or length raises ValueError, an id outside its table
    IndexError (as transformers' embedding lookup does)."""
    if input_ids.dim() != 2:
        raise ValueError(f"input_ids [B, Lt] expected, got {tuple(input_ids.shape)}")
    B, Lt = input_ids.shape
    if Lt > cfg["max_position_embeddings"]:
        raise ValueError(f"{Lt} text tokens exceed max_position_embeddings = {cfg['max_position_embeddings']}")
    for name, t, hi in (("input_ids", input_ids, cfg["vocab_size"]), ("token_type_ids", token_type_ids, cfg["type_vocab_size"])):
        check_ids(name, t, (B, Lt), hi)


def check_ids(name, t, shape, hi):
    """One integer id tensor (or None): the shape, then every entry in [0, hi)."""
    if t is None:
        return
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    lo_, hi_ = int(t.min()), int(t.max())
    if lo_ < 0 or hi_ >= hi:
        raise IndexError(f"{name} must lie in [0, {hi}): found {lo_}..{hi_}")


# ---- (name, shape) of the tensors of a BERT layer, in transformers' state-dict order ----
def attention_spec(p, H, ctx=None):
    ctx = H if ctx is None else ctx
    return [(p + ".query.weight", (H, H)), (p + ".query.bias", (H,)), (p + ".key.weight", (H, ctx)), (p + ".key.bias", (H,)),
            (p + ".value.weight", (H, ctx)), (p + ".value.bias", (H,))]


def dense_ln_spec(p, n_in, n_out):
    return [(p + ".dense.weight", (n_out, n_in)), (p + ".dense.bias", (n_out,)), (p + ".LayerNorm.weight", (n_out,)),
            (p + ".LayerNorm.bias", (n_out,))]


def bert_layer_spec(p, H, I):
    return (attention_spec(p + ".attention.self", H) + dense_ln_spec(p + ".attention.output", H, H) +
            [(p + ".intermediate.dense.weight", (I, H)), (p + ".intermediate.dense.bias", (I,))] + dense_ln_spec(p + ".output", I, H))


# ---- replay against a captured call: plain functions of (names, static, new), so they run on CPU tensors ----------------------------
def check_against_captured(names, static, new):
    """`new`, the inputs of a replay, against `static`, the buffers of the captured call: None where that call had None, a tensor
    of the same shape where it had a tensor.  `Tensor.copy_` alone would broadcast [1, L] into a [B, L] buffer."""
    for name, s, n in zip(names, static, new):
        if (s is None) != (n is None) or (s is not None and tuple(s.shape) != tuple(n.shape)):
            raise ValueError(f"replay: {name} differs from the captured call (None or another shape)")


def refill(static, new):
    """The new values into the captured buffers; what was None at capture stays None."""
    for s, n in zip(static, new):
        if s is not None:
            s.copy_(n)


def keep_head(enc, sd, *prefixes):
    """The fp32 host tensors of a head's layers (`<prefix>.weight`, `<prefix>.bias`) into `enc._head`, by state-dict key, beside
    their packed copies: a few MB, where `HeadTrainer`'s masters start.  A plain function: whatever stands where the encoder
    stands in a wrapper's `load_state_dict` takes it."""
    head = enc.__dict__.setdefault("_head", {})
    for p in prefixes:
        for k in (p + ".weight", p + ".bias"):
            head[k] = np.array(sd[k], np.float32)


class Model:
    """What an encoder and a head wrapper around one have in common as objects."""

    def eval(self):
        return self

    def _check_state_dict(self, sd, want, strict):
        """Strict load: no missing and no unexpected key; always: the shape of every tensor the model takes."""
        if strict:
            missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
            if missing or extra:
                raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing {missing[:4]} unexpected {extra[:4]}")
        for k, shp in want.items():
            if tuple(sd[k].shape) != tuple(shp):
                raise RuntimeError(f"weight '{k}' has shape {tuple(sd[k].shape)}, expected {tuple(shp)}")

    def _load_with_encoder(self, enc, prefix, spec, sd, strict, rekey=None):
        """A head wrapper's `load_state_dict` up to its own tensors: numpy, `rekey(sd)` where key names need work (ViT's hub-era
        names, the tied decoder of the pre-training heads), the strict check of keys and shapes against the wrapper's whole
        `spec`, then the tensors under `prefix` into the encoder.  -> the dict, for the wrapper's own `_load_lin` / `_load_ln`."""
        sd = to_numpy(sd)
        if rekey is not None:
            sd = rekey(sd)
        self._check_state_dict(sd, dict(spec), strict)
        enc.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict)
        return sd


class BertOps(Model):
    """The base of the encoders: the packed weights, the ops over the C ABI, the BERT layer built from them and the front."""

    _INPUTS = ()                             # the tensors a call takes, in the order of `__call__`, `_check`, `_forward` and `_embed`

    def __init__(self, config, precision="bf16", device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError(f"vltk_amd.{type(self).__name__} needs a GPU: there is no CPU fallback")
        L.load()
        self.cfg = dict(config)
        self.dt, self.tdt = DTYPES[precision]
        self.device = torch.device(device)
        self.es = 4 if precision == "fp32" else 2
        self.ktile = 128 // self.es                    # elements per 128-byte K-tile of the GEMM
        self._lin, self._ln, self._tab = {}, {}, {}
        self._loaded = False

    # ---- weights -------------------------------------------------------------------------------------------
    def _pack(self, w, b):
        """nn.Linear weight [N, K] (+ bias) -> device (packed rows padded to the K-tile, f32 bias)."""
        N, K = w.shape
        Kp = (K + self.ktile - 1) // self.ktile * self.ktile
        wk = np.zeros((N, Kp), np.float32)
        wk[:, :K] = w
        wp, bp = pack(wk, self.dt, bias=b)
        return torch.from_numpy(wp).to(self.device), torch.from_numpy(bp).to(self.device), N, Kp

    def _load_lin(self, sd, name, *parts):   # one GEMM for several nn.Linear applied to the same input (rows concatenated)
        w = np.concatenate([sd[p + ".weight"] for p in parts], 0)
        b = np.concatenate([sd[p + ".bias"] for p in parts], 0)
        self._lin[name] = self._pack(w, b)

    def _load_ln(self, sd, name):
        self._ln[name] = (torch.from_numpy(sd[name + ".weight"]).to(self.device), torch.from_numpy(sd[name + ".bias"]).to(self.device))

    def _load_tab(self, sd, name):            # embedding tables stay in the storage type
        self._tab[name] = torch.from_numpy(sd[f"embeddings.{name}.weight"]).to(self.device).to(self.tdt).contiguous()

    def _load_att_self(self, sd, p):          # q, k, v of a self-attention share the input: one GEMM
        self._load_lin(sd, p + ".qkv", p + ".query", p + ".key", p + ".value")

    def _load_bert_layer(self, sd, p):
        self._load_att_self(sd, p + ".attention.self")
        self._load_lin(sd, p + ".attention.output.dense", p + ".attention.output.dense")
        self._load_ln(sd, p + ".attention.output.LayerNorm")
        self._load_lin(sd, p + ".intermediate.dense", p + ".intermediate.dense")
        self._load_lin(sd, p + ".output.dense", p + ".output.dense")
        self._load_ln(sd, p + ".output.LayerNorm")

    def _require_loaded(self):
        if not self._loaded:
            raise RuntimeError(f"{type(self).__name__}: load_state_dict() first")

    # ---- ops (each one call into the C ABI) ----------------------------------------------------------------------
    def _linear(self, x, name, act=L.VK_ACT_NONE, residual=None):
        w, b, N, Kp = self._lin[name]
        M, K = x.shape
        if K != Kp:                                     # box_fc: K = 4 -> one zero-padded K-tile (layout only)
            xp = torch.zeros((M, Kp), dtype=x.dtype, device=self.device)
            xp[:, :K] = x
            x = xp
        ldy = (N + 7) // 8 * 8
        y = torch.empty((M, ldy), dtype=self.tdt, device=self.device)
        L.call("vk_linear", x.data_ptr(), M, Kp, w.data_ptr(), b.data_ptr(), residual.data_ptr() if residual is not None else None,
               y.data_ptr(), N, ldy, act, self.dt, self.dt, stream(self.device))
        return y if ldy == N else y[:, :N]

    def _layernorm(self, x, name, out=None, scale=1.0, accumulate=False):
        g, b = self._ln[name]
        M, Cc = x.shape
        y = torch.empty((M, Cc), dtype=self.tdt, device=self.device) if out is None else out
        L.call("vk_layernorm", x.data_ptr(), x.stride(0), g.data_ptr(), b.data_ptr(), y.data_ptr(), y.stride(0), M, Cc, self.cfg.get("layer_norm_eps", LN_EPS), scale,
               int(accumulate), self.dt, stream(self.device))
        return y

    def attention_entry(self, Lq, Lk, ldq, ldk, ldv, aligned, route=True):
        """The entry point a forward calls for one attention and the kernel that runs there: (name, VK_ATT_ROUTE_*).  16-bit: the
        small matrix-core kernel through vk_attention where it reaches (20 / 36 tokens), vk_attention_tiled at every other length;
        fp32 stays on vk_attention (the LDS kernel where a head fits it, the streaming kernel beyond).  `route=False` leaves out the
        library calls that only name the kernel (the route is then None unless the rule itself had to ask)."""
        d = self.cfg["hidden_size"] // self.cfg["num_attention_heads"]

        def ask(tiled_entry):
            return L.load().vk_attention_route(Lq, Lk, d, self.dt, ldq, ldk, ldv, int(aligned), tiled_entry)
        if self.dt == L.VK_F32:
            return "vk_attention", (ask(0) if route else None)
        r = ask(0)
        if r == L.VK_ATT_ROUTE_MFMA:
            return "vk_attention", r
        return "vk_attention_tiled", (ask(1) if route else None)

    def _attention(self, q, k, v, mask, B, Lq, Lk):
        H, heads = self.cfg["hidden_size"], self.cfg["num_attention_heads"]
        out = torch.empty((B * Lq, H), dtype=self.tdt, device=self.device)
        aligned = (q.data_ptr() | k.data_ptr() | v.data_ptr()) % 16 == 0
        name, _ = self.attention_entry(Lq, Lk, q.stride(0), k.stride(0), v.stride(0), aligned, route=False)
        L.call(name, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
               mask.data_ptr() if mask is not None else None, out.data_ptr(), H, B, heads, Lq, Lk, H // heads, self.dt, stream(self.device))
        return out

    def _gather_rows(self, x, idx):
        """Rows `idx` (int32, on the device) of contiguous `x [M, C]` -> [len(idx), C].  The kernel copies 16-byte lanes."""
        n, Cc = idx.numel(), x.shape[1]
        if Cc * self.es % 16:
            raise ValueError(f"gather of rows of {Cc} elements: their size must be a multiple of 16 bytes")
        rows = torch.empty((n, Cc), dtype=self.tdt, device=self.device)
        L.call("vk_gather_rows", x.data_ptr(), idx.data_ptr(), n, Cc * self.es, rows.data_ptr(), stream(self.device))
        return rows

    # ---- layers (modeling_lxmert.py) -----------------------------------------------------------------------------
    def _self_att_block(self, p, x, mask, B, Lx):       # LxmertSelfAttentionLayer :298-316
        H = self.cfg["hidden_size"]
        qkv = self._linear(x, p + ".self.qkv")
        ctx = self._attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask, B, Lx, Lx)
        t = self._linear(ctx, p + ".output.dense", residual=x)
        return self._layernorm(t, p + ".output.LayerNorm")

    def _ffn(self, inter, outp, x):                     # LxmertIntermediate + LxmertOutput :319-342
        h = self._linear(x, inter + ".dense", act=L.VK_ACT_GELU)
        t = self._linear(h, outp + ".dense", residual=x)
        return self._layernorm(t, outp + ".LayerNorm")

    def _bert_layer(self, p, x, mask, B, Lx):           # LxmertLayer :345-358
        a = self._self_att_block(p + ".attention", x, mask, B, Lx)
        return self._ffn(p + ".intermediate", p + ".output", a)

    def _hidden_after(self, n_layers, *inputs):
        """The single-stream encoders (`_embed`, layers `encoder.layer.i`) stopped after layer `n_layers - 1`: -> (its rows
        [B * L, H], the additive mask or None).  `EncoderTrainer` runs the frozen layers through it; `_forward` does not."""
        x, mask = self._embed(*inputs)
        B = inputs[0].shape[0]
        Lx = x.shape[0] // B
        for i in range(n_layers):
            x = self._bert_layer(f"encoder.layer.{i}", x, mask, B, Lx)
        return x, mask

    def _pooler(self, x, B, Lx):                        # LxmertPooler :566-572: tanh(dense(first token of each sequence))
        w, bb, N, Kp = self._lin["pooler.dense"]        # the first rows are picked by a stride-Lx 1x1 "convolution"
        H = self.cfg["hidden_size"]
        pooled = torch.empty((B, H), dtype=self.tdt, device=self.device)
        L.call("vk_conv2d", x.data_ptr(), B, Lx, 1, H, w.data_ptr(), bb.data_ptr(), None, pooled.data_ptr(), H, H, 1, 1, Lx, 0, 1, 1,
               L.VK_ACT_TANH, self.dt, self.dt, stream(self.device))
        return pooled

    # ---- the front: what stands between a caller and `_forward` --------------------------------------------------------------
    # An encoder supplies `_INPUTS`, `_check(*inputs, **options)` (host-side: everything that needs the VALUES of an input, so it
    # runs before a launch or a capture, never inside one), `_forward(*inputs)`, and where it has them `_embed` and `_before_capture`.
    def _run(self, forward, inputs, **options):
        """One eager call, of the encoder or of a head over it: check -> `forward(*inputs)` -> synchronize."""
        self._check(*inputs, **options)
        out = forward(*inputs)
        torch.cuda.synchronize(self.device)
        return out

    def _before_capture(self, *inputs):
        """Host work that a forward of these inputs does once and keeps (ViT: the position table of the grid)."""

    def _capture_inputs(self, inputs, **options):
        """Capture one forward for the SHAPES of `inputs` into a HIP graph -> `run(new)`: refuses inputs that differ from the
        captured call's in None or shape, repeats the host check, copies them into the captured buffers, launches the graph and
        returns the (static) output tensors.  An input that was None at capture stays at its default."""
        self._check(*inputs, **options)
        self._require_loaded()
        self._before_capture(*inputs)
        static = [None if a is None else a.to(self.device).clone() for a in inputs]
        graph, outs = self._capture(self._forward, static)

        def run(new):
            check_against_captured(self._INPUTS, static, new)
            self._check(*new, **options)
            refill(static, new)
            graph.replay()
            return outs
        return run

    def _capture(self, forward, static_inputs):
        """`forward(*static_inputs)` once on a side stream (one-time attribute / lazy-init calls must not be captured), then
        captured into a HIP graph -> (graph, the static output tensors)."""
        dev = self.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            forward(*static_inputs)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = forward(*static_inputs)
        return graph, outs

"""torch <-> C-ABI glue for one rendering pass: descriptor, parameter packing, autograd.Function.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); all arithmetic of the hot
path runs in libsnerf_hip.so.  There is no fallback: a CPU tensor or a missing library raises.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

import os
import weakref

_WS_POISON = os.environ.get("SNERF_WS_POISON", "0") == "1"
_WS_POISON_BYTE = 0xFF      # the fill of _poison / lease_workspace: 0xFF is NaN in fp16 / fp32 / fp64 and -1 as an integer (tests set others)

from . import _lib

# SNERF_MFMA=f16x2|f16x1 overrides every ModelSpec.mfma (diagnostics); unset, ModelSpec.mfma decides and its default is f16x2 --
# the arithmetic a C caller gets with no arithmetic flag
BASE_FLAGS = _lib.MFMA_FLAGS.get(os.environ.get("SNERF_MFMA", "").lower())


DEFAULT_MFMA = "f16x2"


def mfma_mode(pipeline_cfg=None, run_cfg=None) -> str:
    """Matrix-unit arithmetic of the dense layers from the reference's two precision knobs:
    `precision` (baseline/pipelines/nerf.py:65, handed to the trainer at framework/pipelines.py:319; 16 = half precision) and the
    run config's `float32_matmul_precision` (framework/configs.py:26, applied at framework/pipelines.py:254-256).  The build adds
    the pipeline field `mfma_precision`:
      "f16x2" (default)  two fp16 planes of block-scaled operands (22 significant bits), three products: fp32-class results
      "f16x1" / "bf16"   REDUCED precision: ONE fp16 plane of the same block-scaled tensors (11 significant bits -- the operand
                         precision of TF32, three bits more than bf16), one product, half the activation bytes.  `precision = 16`
                         selects it; "bf16" is the name BASELINE.json's configs[2] / [4] use and maps to the same mode
      "auto"             follow float32_matmul_precision: "highest" -> f16x2; "high" (TF32-class on the reference's hardware) and
                         "medium" -> f16x1"""
    mode = getattr(pipeline_cfg, "mfma_precision", DEFAULT_MFMA)
    if getattr(pipeline_cfg, "precision", 32) == 16:
        return "f16x1"
    if mode == "auto":
        return {"highest": "f16x2", "high": "f16x1", "medium": "f16x1"}[
            getattr(run_cfg, "float32_matmul_precision", "highest")]
    return "f16x1" if mode == "bf16" else mode

# parameter names in the reference's state_dict order -> SnerfParams field
_HEAD_FIELDS = {
    "sigma_from_xyz.0.weight": "sigma_w", "sigma_from_xyz.0.bias": "sigma_b",
    "feats_from_xyz.weight": "feats_w", "feats_from_xyz.bias": "feats_b",
    "rgb_from_xyzdir.0.weight": "rgb_w0", "rgb_from_xyzdir.0.bias": "rgb_b0",
    "rgb_from_xyzdir.2.weight": "rgb_w2", "rgb_from_xyzdir.2.bias": "rgb_b2",
    "semantic_prediction.0.weight": "sem_w0", "semantic_prediction.0.bias": "sem_b0",
    "semantic_prediction.2.weight": "sem_w2", "semantic_prediction.2.bias": "sem_b2",
    "sky_color.0.weight": "sky_w0", "sky_color.0.bias": "sky_b0",
    "sky_color.2.weight": "sky_w2", "sky_color.2.bias": "sky_b2",
    "beta_from_xyz.0.weight": "beta_w0", "beta_from_xyz.0.bias": "beta_b0",
    "beta_from_xyz.2.weight": "beta_w2", "beta_from_xyz.2.bias": "beta_b2",
    "semantic_beta_from_xyz.0.weight": "sbeta_w0", "semantic_beta_from_xyz.0.bias": "sbeta_b0",
    "semantic_beta_from_xyz.2.weight": "sbeta_w2", "semantic_beta_from_xyz.2.bias": "sbeta_b2",
}


@dataclass(frozen=True)
class ModelSpec:
    """Architecture part of SnerfDesc (field names: configs/pipelines/rs_semantic.toml:13-67)."""
    fc_units: int = 512
    fc_layers: int = 8
    feat_last: int = 256
    fc_skips: tuple = (4,)
    n_freq: int = 10            # mapping_pos_n_freq; 0 = identity (baseline SatNeRF)
    siren: bool = True
    t_dim: int = 4
    n_classes: int = 5          # 0 = baseline SatNeRF
    sem_sigmoid: bool = True
    use_tj_instead_of_beta: bool = False
    use_tj_for_s: bool = False
    use_separate_beta_for_s: bool = False
    use_separate_tj_for_semantic: bool = False
    mfma: str = "f16x2"         # see mfma_mode()

    @staticmethod
    def from_pipeline_cfg(pc, n_classes: int, model: str = "semantic", run_cfg=None) -> "ModelSpec":
        sem = model == "semantic"
        W = pc.fc_units
        return ModelSpec(
            fc_units=W, fc_layers=pc.fc_layers, feat_last=W if pc.fc_use_full_features else W // 2,
            fc_skips=tuple(pc.fc_skips), n_freq=pc.mapping_pos_n_freq if sem else 0,
            siren=pc.activation_function == "siren", t_dim=pc.t_embedding_tau,
            n_classes=n_classes if sem else 0,
            sem_sigmoid=sem and getattr(pc, "semantic_activation_function", "sigmoid") == "sigmoid",
            use_tj_instead_of_beta=sem and bool(getattr(pc, "use_tj_instead_of_beta", False)),
            use_tj_for_s=sem and bool(getattr(pc, "use_tj_for_s", False)),
            use_separate_beta_for_s=sem and bool(getattr(pc, "use_separate_beta_for_s", False)),
            use_separate_tj_for_semantic=sem and bool(getattr(pc, "use_separate_tj_for_semantic", False)),
            mfma=mfma_mode(pc, run_cfg))

    def desc(self, n_rays: int, n_samples: int, flags: int = 0) -> _lib.SnerfDesc:
        mask = 0
        for s in self.fc_skips:
            mask |= 1 << int(s)
        return _lib.SnerfDesc(
            n_rays=n_rays, n_samples=n_samples, fc_units=self.fc_units, fc_layers=self.fc_layers,
            feat_last=self.feat_last, skip_mask=mask, n_freq=self.n_freq, siren=int(self.siren), t_dim=self.t_dim,
            n_classes=self.n_classes, sem_sigmoid=int(self.sem_sigmoid),
            use_tj_instead_of_beta=int(self.use_tj_instead_of_beta), use_tj_for_s=int(self.use_tj_for_s),
            use_separate_beta_for_s=int(self.use_separate_beta_for_s),
            use_separate_tj_for_semantic=int(self.use_separate_tj_for_semantic), flags=flags | (_lib.MFMA_FLAGS[self.mfma] if BASE_FLAGS is None else BASE_FLAGS))

    def param_names(self) -> list:
        names = []
        for i in range(self.fc_layers):
            names += [f"fc_net.{2 * i}.weight", f"fc_net.{2 * i}.bias"]
        names += ["sigma_from_xyz.0.weight", "sigma_from_xyz.0.bias", "feats_from_xyz.weight", "feats_from_xyz.bias",
                  "rgb_from_xyzdir.0.weight", "rgb_from_xyzdir.0.bias", "rgb_from_xyzdir.2.weight",
                  "rgb_from_xyzdir.2.bias"]
        if self.n_classes > 0:
            names += ["semantic_prediction.0.weight", "semantic_prediction.0.bias", "semantic_prediction.2.weight",
                      "semantic_prediction.2.bias"]
        for j in (0, 2, 4, 6):
            names += [f"sun_v_net.{j}.weight", f"sun_v_net.{j}.bias"]
        names += ["sky_color.0.weight", "sky_color.0.bias", "sky_color.2.weight", "sky_color.2.bias",
                  "beta_from_xyz.0.weight", "beta_from_xyz.0.bias", "beta_from_xyz.2.weight", "beta_from_xyz.2.bias"]
        if self.n_classes > 0 and self.use_separate_beta_for_s:
            names += ["semantic_beta_from_xyz.0.weight", "semantic_beta_from_xyz.0.bias",
                      "semantic_beta_from_xyz.2.weight", "semantic_beta_from_xyz.2.bias"]
        return names


def _poison(t):
    """with SNERF_WS_POISON=1 (diagnostic) a fresh tensor is filled with _WS_POISON_BYTE bytes (0xFF), so that a kernel which reads
    bytes nobody wrote shows up as NaN / a wild value instead of depending on what the allocator happens to hand out"""
    if _WS_POISON and t.numel():
        t.view(torch.uint8).fill_(_WS_POISON_BYTE)
    return t


def _empty(*a, **k):
    return _poison(torch.empty(*a, **k))


# ---- pass workspaces -------------------------------------------------------------------------------------------------
# A training pass needs 8-20 GB of workspace between its forward and its backward.  Taking it from torch's caching allocator
# every step works until something else is allocated while the block lies free: the allocator carves a few MB for a result
# tensor out of the free 10 GB block, the next forward finds no block of its size and goes to hipMalloc (10 GB: milliseconds
# on a quiet box, a quarter of a second on a busy one) in the middle of training.  Workspaces are therefore LEASED from a pool
# of whole tensors keyed by (device, stream, size): a lease ends in the pass's backward (or when its autograd node dies) and the
# same tensor serves the same pass of the next step on the same stream, so stream order alone makes the reuse safe.
_WS_FREE: dict = {}                 # (device index, stream id, nbytes) -> [tensor, ...]
_WS_FREE_BYTES = 0
_WS_POOL_CAP = int(float(os.environ.get("SNERF_WS_POOL_GB", "96")) * (1 << 30))   # idle bytes kept; beyond it the oldest idle workspaces go back to torch


class _WsLease:
    __slots__ = ("key", "t")

    def __init__(self, key, t):
        self.key, self.t = key, t

    def release(self):
        global _WS_FREE_BYTES
        t, self.t = self.t, None
        if t is None:
            return
        _WS_FREE.setdefault(self.key, []).append(t)
        _WS_FREE_BYTES += t.numel()
        while _WS_FREE_BYTES > _WS_POOL_CAP and _WS_FREE:
            k = next(iter(_WS_FREE))          # dicts keep insertion order: the key idle for longest first
            lst = _WS_FREE[k]
            _WS_FREE_BYTES -= lst.pop(0).numel()
            if not lst:
                del _WS_FREE[k]

    def __del__(self):
        try:
            self.release()
        except Exception:      # interpreter shutdown: the module's globals may be gone
            pass


def lease_workspace(dev, nbytes: int) -> _WsLease:
    global _WS_FREE_BYTES
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream, int(nbytes))
    lst = _WS_FREE.get(key)
    if lst:
        t = lst.pop()
        _WS_FREE_BYTES -= t.numel()
        if not lst:
            del _WS_FREE[key]
        if _WS_POISON:
            t.fill_(_WS_POISON_BYTE)
    else:
        try:
            t = _empty(nbytes, dtype=torch.uint8, device=dev)
        except torch.cuda.OutOfMemoryError:
            # the idle workspaces of other shapes / streams live outside torch's allocator: give them back and try once more
            release_workspaces()
            torch.cuda.empty_cache()
            t = _empty(nbytes, dtype=torch.uint8, device=dev)
    return _WsLease(key, t)


def release_workspaces():
    """hand every idle workspace back to torch's allocator (before a phase with another memory profile, e.g. full-frame inference)"""
    global _WS_FREE_BYTES
    _WS_FREE.clear()
    _WS_FREE_BYTES = 0


# ---- gradient sinks -------------------------------------------------------------------------------------------------
# A parameter may have a registered SINK: a preallocated gradient tensor (FlatAdam's view into its flat bucket, which is
# also p.grad).  A pass whose parameters all have one accumulates its packed gradients straight into the sinks
# (snerf_unpack_grads, accumulate = 1) and returns no parameter gradients to autograd -- the 2 x 23 AccumulateGrad add
# kernels per step (main + solar-correction pass, each parameter) disappear.  The two passes run their backward on
# different HIP streams, so the unpack launches are chained by events (each waits for the previous one; with two
# contributions the sum is the same in either order).  Parameters without sinks (tests, foreign optimisers) get their
# gradients from autograd as before.  SNERF_GRAD_SINKS=0 switches the mechanism off (A/B).
_GRAD_SINKS: dict = {}      # id(parameter) -> (weakref, sink tensor)
_SINK_EVENT: dict = {}      # device index -> event of the last accumulating unpack
_SINK_TOUCHED: set = set()  # ids of parameters whose sink a pass has accumulated into (cleared by the optimiser's zero_grad)
_SINKS_ON = os.environ.get("SNERF_GRAD_SINKS", "1") != "0"


def register_grad_sinks(params, sinks):
    for p, g in zip(params, sinks):
        _GRAD_SINKS[id(p)] = (weakref.ref(p), g)


def unregister_grad_sinks(params):
    for p in params:
        _GRAD_SINKS.pop(id(p), None)


def wait_grad_sinks(device=None):
    """Make the current stream wait for the last accumulating unpack.  A pass that writes sinks hands autograd no parameter
    gradients, so the engine's end-of-backward stream synchronisation (which follows AccumulateGrad) does not cover the
    side stream of the solar-correction pass: every consumer of the sink tensors calls this first (FlatAdam does)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ev = _SINK_EVENT.get(dev.index if dev.index is not None else torch.cuda.current_device())
    if ev is not None:
        torch.cuda.current_stream(dev).wait_event(ev)


_SINK_SYNC_QUEUED: set = set()


def _queue_sink_sync(dev):
    """Once per backward(): when the whole graph has run, the stream that called backward() waits for the last sink write
    (autograd's own end-of-backward synchronisation only follows AccumulateGrad nodes, which the sink path bypasses)."""
    key = dev.index
    if key in _SINK_SYNC_QUEUED:
        return

    def _cb():
        _SINK_SYNC_QUEUED.discard(key)
        wait_grad_sinks(dev)

    try:
        torch.autograd.Variable._execution_engine.queue_callback(_cb)
        _SINK_SYNC_QUEUED.add(key)
    except RuntimeError:      # not inside a backward pass of the engine (direct call): the consumer synchronises
        pass


_SINKS_ACTIVE = False


class accumulate_into_sinks:
    """`with ops.accumulate_into_sinks(): loss.backward()` -- only inside this context do the passes add their parameter
    gradients straight into the registered sink tensors (and hand autograd None for them).  It is the training loop's
    statement that this backward is a plain accumulate-into-.grad one.  Anywhere else -- torch.autograd.grad,
    backward(inputs=...), gradient checks -- the passes return ordinary gradients and touch no .grad.  Entering also
    discards a stale end-of-backward marker that a backward which raised may have left behind."""

    def __enter__(self):
        global _SINKS_ACTIVE
        self._prev = _SINKS_ACTIVE
        _SINKS_ACTIVE = True
        _SINK_SYNC_QUEUED.clear()
        return self

    def __exit__(self, *exc):
        global _SINKS_ACTIVE
        _SINKS_ACTIVE = self._prev
        _SINK_SYNC_QUEUED.clear()
        return False


def _sinks_for(params):
    if not _SINKS_ON or not _SINKS_ACTIVE or not _GRAD_SINKS:
        return None
    out = []
    for p in params:
        e = _GRAD_SINKS.get(id(p))
        if e is None or e[0]() is not p or p.grad is None or p.grad.data_ptr() != e[1].data_ptr():
            return None      # not (or no longer) wired to its sink: autograd accumulates
        out.append(e[1])
    return out


def _check_dev(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"snerf_amd: '{name}' must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"snerf_amd: '{name}' must be float32, got {t.dtype}")


def params_struct(spec: ModelSpec, tensors: dict) -> _lib.SnerfParams:
    ps = _lib.SnerfParams()
    for name in spec.param_names():
        t = tensors[name]
        _check_dev(t, name)
        if not t.is_contiguous():
            raise RuntimeError(f"snerf_amd: parameter '{name}' must be contiguous")
        if name.startswith("fc_net."):
            i = int(name.split(".")[1]) // 2
            (ps.fc_w if name.endswith("weight") else ps.fc_b)[i] = t.data_ptr()
        elif name.startswith("sun_v_net."):
            j = int(name.split(".")[1]) // 2
            (ps.sun_w if name.endswith("weight") else ps.sun_b)[j] = t.data_ptr()
        else:
            setattr(ps, _HEAD_FIELDS[name], t.data_ptr())
    return ps


def pack_params(spec: ModelSpec, tensors: dict) -> torch.Tensor:
    """state_dict tensors -> packed MFMA-friendly buffer (snerf_pack_params)."""
    d = spec.desc(1, 1)
    dev = tensors[spec.param_names()[0]].device
    packed = _empty(_lib.call_size("snerf_packed_floats", d), dtype=torch.float32, device=dev)
    _lib.call("snerf_pack_params", d, params_struct(spec, tensors), packed)
    return packed


def unpack_grads(spec: ModelSpec, packed_grads: torch.Tensor, like: dict, accumulate_into: dict | None = None) -> dict:
    """packed gradient buffer -> dict name -> gradient tensor shaped like the parameters."""
    d = spec.desc(1, 1)
    if accumulate_into is None:
        grads = {n: _poison(torch.empty_like(like[n])) for n in spec.param_names()}
    else:
        grads = accumulate_into
    _lib.call("snerf_unpack_grads", d, packed_grads, params_struct(spec, grads), accumulate_into is not None)
    return grads


@dataclass
class PassInputs:
    """One ray batch in either of the two seams (renderer: rays [+u]; inference(): xyz + z_vals)."""
    sun_d: torch.Tensor | None = None     # (N,3) (may be a strided view into extras (N,4)); None only for a geometry pass, which reads no sun
    rays: torch.Tensor | None = None      # (N,8)
    xyz: torch.Tensor | None = None       # (N,S,3)
    z_vals: torch.Tensor | None = None    # (N,S)
    z_steps: torch.Tensor | None = None   # (S)
    u: torch.Tensor | None = None         # (N,S)
    _keep: list = field(default_factory=list)

    def struct(self, t, t_s):
        si = _lib.SnerfInputs()
        for name in ("rays", "xyz", "z_vals", "z_steps", "u"):
            v = getattr(self, name)
            if v is not None:
                _check_dev(v, name)
                v = v.contiguous()
                self._keep.append(v)
                setattr(si, name, v.data_ptr())
        sd = self.sun_d
        si.sun_stride = 3
        if sd is not None:      # (the library names a missing sun_d / t itself, for every pass but the geometry pass)
            _check_dev(sd, "sun_d")
            if sd.dim() != 2 or sd.shape[1] != 3 or sd.stride(1) != 1:
                sd = sd.contiguous()
            self._keep.append(sd)
            si.sun_d = sd.data_ptr()
            si.sun_stride = sd.stride(0) if sd.shape[0] > 1 else 3
        si.t = t.data_ptr() if t is not None else None
        si.t_s = t_s.data_ptr() if t_s is not None else None
        return si

    def n_rays(self) -> int:
        """N from whichever per-ray tensor the batch carries"""
        for v in (self.rays, self.z_vals, self.xyz, self.u, self.sun_d):
            if v is not None:
                return int(v.shape[0])
        raise ValueError("PassInputs: no per-ray tensor to take the number of rays from")


_OUT_SHAPES = {
    "rgb": lambda N, S, C: (N, 3), "depth": lambda N, S, C: (N,), "weights": lambda N, S, C: (N, S),
    "transparency": lambda N, S, C: (N, S), "albedo": lambda N, S, C: (N, S, 3), "sun": lambda N, S, C: (N, S, 1),
    "sky": lambda N, S, C: (N, S, 3), "beta": lambda N, S, C: (N, S, 1), "sigmas": lambda N, S, C: (N, S),
    "beta_semantic": lambda N, S, C: (N, S, 1), "semantic_logits": lambda N, S, C: (N, C),
}


def output_keys(spec: ModelSpec, sc_pass: bool) -> list:
    if sc_pass:
        return ["weights", "transparency", "sun"]
    keys = ["rgb", "depth", "weights", "transparency", "albedo", "sun", "sky", "beta", "sigmas"]
    if spec.n_classes > 0:
        if spec.use_separate_beta_for_s:
            keys.append("beta_semantic")
        keys.append("semantic_logits")
    return keys


def _forward_setup(spec, pin, t, t_s, flags, n_samples=None):
    """What every forward entry does before it allocates: S from the inputs (`n_samples`: a relight, whose inputs carry no depths),
    the descriptor, the workspace size, contiguous t / t_s and the inputs struct.  Returns (S, desc, workspace bytes, tc, tsc,
    launch); launch(packed, so, ws) is the snerf_forward call on the workspace tensor `ws`."""
    S = int(n_samples) if n_samples is not None else (
        pin.z_vals.shape[1] if pin.z_vals is not None else (pin.u.shape[1] if pin.u is not None else pin.z_steps.shape[0]))
    d = spec.desc(t.shape[0] if t is not None else pin.n_rays(), S, flags)      # (t = None: a geometry pass, which reads no embedding)
    nbytes = _lib.call_size("snerf_workspace_bytes", d)
    if t is not None:
        _check_dev(t, "t")
    tc = t.contiguous() if t is not None else None
    tsc = t_s.contiguous() if t_s is not None else None
    si = pin.struct(tc, tsc)
    return S, d, nbytes, tc, tsc, lambda packed, so, ws: _lib.call("snerf_forward", d, packed, si, so, ws, ws.numel())


class _RenderPass(torch.autograd.Function):
    """forward = snerf_forward, backward = snerf_backward (+ snerf_unpack_grads).  A backward in which no parameter needs a
    gradient (frozen network, the leaf is t / t_s: fitting an image's embedding) is the library's embedding-only backward,
    SNERF_FLAG_EMBED_GRAD: d_t / d_t_s with the bits of the full backward, no gradient buffer, no unpack."""

    @staticmethod
    def forward(ctx, spec, pin, sc_pass, need_grad, packed, names, t, t_s, *params):
        N, dev = t.shape[0], t.device
        flags = (_lib.FLAG_TRAIN if need_grad else 0) | (_lib.FLAG_SC_PASS if sc_pass else 0)
        S, d, nbytes, tc, tsc, launch = _forward_setup(spec, pin, t, t_s, flags)
        with torch.cuda.device(dev):
            lease = lease_workspace(dev, nbytes)
        keys = output_keys(spec, sc_pass)
        outs = {k: _empty(_OUT_SHAPES[k](N, S, spec.n_classes), dtype=torch.float32, device=dev) for k in keys}
        label = _empty((N,), dtype=torch.int64, device=dev) if (spec.n_classes > 0 and not sc_pass) else None
        so = _lib.SnerfOutputs()
        for k, v in outs.items():
            setattr(so, k, v.data_ptr())
        so.semantic_label = label.data_ptr() if label is not None else None
        if pin.z_vals is not None and pin.z_vals.is_contiguous() and pin.z_vals.dtype == torch.float32:
            # depths given: they ARE the result (no copy-out launch).  ALIASING: results["z_vals"] shares storage with the caller's
            # tensor -- in fused_model_rendering the main pass's result, the sc pass's input and its result are one buffer, which
            # the backward passes read again.  Never edit it in place (tests/test_gpu_kernels.py pins the contract).
            z_out = pin.z_vals.detach()
        else:
            z_out = _empty((N, S), dtype=torch.float32, device=dev)
            so.z_vals = z_out.data_ptr()
        launch(packed, so, lease.t)
        if not need_grad:
            lease.release()    # nothing is kept for a backward: the next pass of this size on this stream may have it
        ctx.spec, ctx.pin, ctx.desc, ctx.lease, ctx.nbytes = spec, pin, d, lease, nbytes
        ctx.packed, ctx.names, ctx.keys, ctx.tc, ctx.tsc = packed, names, keys, tc, tsc
        ctx.param_like = params
        ctx.train = need_grad
        ctx.set_materialize_grads(False)   # results the loss does not use arrive as None, not as zero tensors
        ret = tuple(outs[k] for k in keys)
        nd = [z_out] + ([label] if label is not None else [])
        ctx.mark_non_differentiable(*nd)
        ctx.n_diff = len(keys)
        return ret + tuple(nd)

    @staticmethod
    def backward(ctx, *gouts):
        if not ctx.train:
            raise RuntimeError("snerf_amd: backward through a pass that was run without SNERF_FLAG_TRAIN")
        spec, d = ctx.spec, ctx.desc
        if ctx.lease.t is None:
            raise RuntimeError("snerf_amd: second backward through one pass (its workspace went back to the pool after the first)")
        go = _lib.SnerfOutGrads()
        keep, live = [], []
        for k, g in zip(ctx.keys, gouts[:ctx.n_diff]):
            if g is not None:
                g = g.contiguous()
                keep.append(g)
                live.append(k)
                setattr(go, k, g.data_ptr())
        if not live:
            return (None,) * (8 + len(ctx.names))
        dev = ctx.tc.device
        d_t = _poison(torch.empty_like(ctx.tc))
        d_ts = _poison(torch.empty_like(ctx.tsc)) if ctx.tsc is not None else None
        if not any(ctx.needs_input_grad[8:]) and _sinks_for(ctx.param_like) is None:
            de = _lib.SnerfDesc.from_buffer_copy(d)
            de.flags |= _lib.FLAG_EMBED_GRAD
            _lib.call("snerf_backward", de, ctx.packed, ctx.pin.struct(ctx.tc, ctx.tsc), go, None, d_t, d_ts, ctx.lease.t, ctx.nbytes)
            ctx.lease.release()
            return (None, None, None, None, None, None, d_t, d_ts) + (None,) * len(ctx.names)
        pg = torch.zeros(_lib.call_size("snerf_grad_floats", d), dtype=torch.float32, device=dev)   # the fp32 region only: the backward touches nothing else
        _lib.call("snerf_backward", d, ctx.packed, ctx.pin.struct(ctx.tc, ctx.tsc), go, pg, d_t, d_ts, ctx.lease.t, ctx.nbytes)
        like = dict(zip(ctx.names, ctx.param_like))
        ctx.lease.release()
        sinks = _sinks_for(ctx.param_like)
        if sinks is not None:
            with torch.cuda.device(dev):
                st = torch.cuda.current_stream()
                prev = _SINK_EVENT.get(dev.index)
                if prev is not None:
                    st.wait_event(prev)
                unpack_grads(spec, pg, like, accumulate_into=dict(zip(ctx.names, sinks)))
                _SINK_TOUCHED.update(id(p) for p in ctx.param_like)
                ev = torch.cuda.Event()
                ev.record(st)
                _SINK_EVENT[dev.index] = ev
            _queue_sink_sync(dev)
            return (None, None, None, None, None, None, d_t, d_ts) + (None,) * len(ctx.names)
        grads = unpack_grads(spec, pg, like)
        # EVERY parameter gets a gradient tensor, zero where no result gradient reaches it: the reference's model returns
        # one concatenated (P, 9 + C) tensor that inference() slices (semantic/models/rs_semantic.py:71-96), so autograd
        # hands e.g. the beta head exact ZEROS (not None) while epoch < first_beta_epoch, and torch.optim.Adam counts
        # those steps (probed on the reference: 45 of 45 parameters have state after one step at epoch 0)
        return (None, None, None, None, None, None, d_t, d_ts) + tuple(grads[n] for n in ctx.names)


def render_pass(spec: ModelSpec, params: dict, pin: PassInputs, t: torch.Tensor, t_s: torch.Tensor | None = None,
                sc_pass: bool = False, packed: torch.Tensor | None = None) -> dict:
    """Run one pass (main, or the solar-correction variant) and return the reference's result dict
    (semantic/models/rs_semantic.py:111-128) plus 'z_vals'.  When `pin.z_vals` is given (contiguous fp32), the returned
    'z_vals' IS that tensor's storage (no copy): do not edit either in place while the pass's backward is pending."""
    names = spec.param_names()
    plist = [params[n] for n in names]
    if packed is None:
        packed = pack_params(spec, params)
    # grad mode is always off inside Function.forward, so decide here whether activations are kept
    need_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in plist) or t.requires_grad
                                             or (t_s is not None and t_s.requires_grad))
    res = _RenderPass.apply(spec, pin, sc_pass, need_grad, packed, names, t, t_s, *plist)
    keys = output_keys(spec, sc_pass)
    out = dict(zip(keys, res[:len(keys)]))
    out["z_vals"] = res[len(keys)]
    if len(res) > len(keys) + 1:
        out["semantic_label"] = res[len(keys) + 1]
    return out


GEOMETRY_KEYS = ("depth", "weights", "transparency", "sigmas", "z_vals")      # the results of a geometry pass (SNERF_FLAG_GEOMETRY)


def _outputs_struct(who, spec, out, N, S, sc_pass=False, geometry=False):
    """SnerfOutputs of the *_into entries: every tensor of `out` checked (a result of this pass; on the GPU; contiguous, of the pass's
    shape and dtype) and bound; every other pointer stays NULL"""
    allowed = set(output_keys(spec, sc_pass)) | {"z_vals"} | ({"semantic_label"} if spec.n_classes > 0 and not sc_pass else set())
    if geometry:
        allowed = set(GEOMETRY_KEYS)
    so = _lib.SnerfOutputs()
    for k, v in out.items():
        if k not in allowed:
            raise KeyError(f"{who}: '{k}' is not a result of this pass (have {sorted(allowed)})")
        want = (N,) if k == "semantic_label" else ((N, S) if k == "z_vals" else _OUT_SHAPES[k](N, S, spec.n_classes))
        if tuple(v.shape) != tuple(want) or not v.is_contiguous():
            raise ValueError(f"{who}: out['{k}'] must be a contiguous {tuple(want)} tensor, got {tuple(v.shape)}")
        if v.dtype != (torch.int64 if k == "semantic_label" else torch.float32):
            raise ValueError(f"{who}: out['{k}'] has dtype {v.dtype}")
        if not v.is_cuda:
            raise RuntimeError(f"snerf_amd: out['{k}'] must live on the GPU (the HIP path has no CPU fallback)")
        setattr(so, k, v.data_ptr())
    return so


DEPTH_MODES = ("mean", "median")      # what a pass's 'depth' is: the expected depth sum w_i z_i, or the median (SNERF_FLAG_DEPTH_MEDIAN)


def _depth_mode_flag(who, depth_mode, out, sc_pass=False):
    """The flag bit of `depth_mode`, checked before anything is sized: an unknown mode and the median of a solar-correction pass
    (which has no depth) are ValueErrors; the median needs 'depth' in `out` (KeyError)."""
    if depth_mode not in DEPTH_MODES:
        raise ValueError(f"{who}: depth_mode must be one of {DEPTH_MODES}, got {depth_mode!r}")
    if depth_mode == "mean":
        return 0
    if sc_pass:
        raise ValueError(f"{who}: depth_mode='median' is not a mode of the solar-correction pass (it has no depth)")
    if "depth" not in out:
        raise KeyError(f"{who}: depth_mode='median' rewrites out['depth'], which `out` does not name")
    return _lib.FLAG_DEPTH_MEDIAN


def _bind_median_scratch(so, out, N, S, dev, scratch):
    """The median launch reads the weights, depths and sigmas the pass hands out (the sigmas so that a ray whose density is not finite
    -- a NaN origin -- gets a NaN depth: the composite gives it zero weights): where `out` does not name one, bind (N, S) views of the flat
    fp32 tensors in `scratch` ('weights' / 'z_vals' / 'sigmas'; made or grown here, so a frame walk that carries the dict allocates them for its
    first chunk only).  Returns the views: hold them until the launch is queued."""
    scratch = scratch if scratch is not None else {}
    held = []
    for k in ("weights", "z_vals", "sigmas"):
        if k in out:
            continue
        buf = scratch.get(k)
        if buf is None or buf.numel() < N * S or buf.device != dev:
            buf = scratch[k] = _empty((N * S,), dtype=torch.float32, device=dev)
        v = buf[:N * S].view(N, S)
        setattr(so, k, v.data_ptr())
        held.append(v)
    return held


@torch.no_grad()
def render_pass_into(spec: ModelSpec, params: dict, pin: PassInputs, t: torch.Tensor, t_s: torch.Tensor | None,
                     out: dict, sc_pass: bool = False, packed: torch.Tensor | None = None,
                     workspace: torch.Tensor | None = None, geometry: bool = False, depth_mode: str = "mean",
                     scratch: dict | None = None) -> torch.Tensor:
    """Inference-only pass that produces ONLY the result tensors named in `out` and writes them in place:
    `out` maps result keys (output_keys(), 'semantic_label', 'z_vals') to preallocated contiguous tensors of the
    pass's shapes -- typically row slices of full-frame buffers, so a chunked render never concatenates
    (eval/utils/util.py:13-42 re-concatenates every key per chunk).  Every other SnerfOutputs pointer stays NULL and
    the composite kernel skips it.  Returns the workspace (pass it back in for the next chunk of the same size).
    `geometry=True` runs the geometry pass (SNERF_FLAG_GEOMETRY): trunk, sigma and the composite, no head launch.  `out` may
    then name GEOMETRY_KEYS only (KeyError otherwise), each with the bits of the full pass; `t`, `t_s` and `pin.sun_d` are not read
    and may be None; a workspace made here is the smaller one of that pass (a larger one given is used as it is).
    `depth_mode="median"` (main or geometry pass) sets SNERF_FLAG_DEPTH_MEDIAN: one launch behind the pass rewrites out['depth'] --
    which `out` must name -- with each ray's median depth, every other result keeping its bits.  That launch reads the pass's weights
    z_vals and sigmas: where `out` names them they are used, otherwise chunk-sized tensors of ops' own, kept in the optional `scratch` dict
    that a caller carries from chunk to chunk."""
    median = _depth_mode_flag("render_pass_into", depth_mode, out, sc_pass)
    if geometry and sc_pass:
        raise ValueError("render_pass_into: geometry=True is a main-pass variant, not one of the solar-correction pass")
    for k in out if geometry else ():      # before anything is sized or allocated
        if k not in GEOMETRY_KEYS:
            raise KeyError(f"render_pass_into(geometry=True): '{k}' is not a result of a geometry pass (have {sorted(GEOMETRY_KEYS)})")
    if t is None and not geometry:
        raise ValueError("render_pass_into: t (N, tau) is required (only a geometry pass reads no embedding)")
    lead = t if t is not None else next(v for v in (pin.rays, pin.z_vals, pin.xyz) if v is not None)      # (t = None: N and the device from the rays)
    N, dev = lead.shape[0], lead.device
    flags = (_lib.FLAG_GEOMETRY if geometry else (_lib.FLAG_SC_PASS if sc_pass else 0)) | median
    S, _, nbytes, _, _, launch = _forward_setup(spec, pin, t, t_s, flags)
    if workspace is None or workspace.numel() < nbytes or workspace.device != dev:
        workspace = _empty(nbytes, dtype=torch.uint8, device=dev)
    so = _outputs_struct("render_pass_into", spec, out, N, S, sc_pass, geometry)
    held = _bind_median_scratch(so, out, N, S, dev, scratch) if median else None
    if packed is None:
        packed = pack_params(spec, params)
    launch(packed, so, workspace)
    del held
    return workspace


def geometry_pass_into(spec: ModelSpec, params: dict, pin: PassInputs, out: dict, packed: torch.Tensor | None = None,
                       workspace: torch.Tensor | None = None, depth_mode: str = "mean", scratch: dict | None = None) -> torch.Tensor:
    """The geometry pass: render_pass_into(geometry=True) without the operands it does not read.  `out` names results of
    GEOMETRY_KEYS -- depth (N), weights / transparency / sigmas / z_vals (N, S) -- each with the bits the full inference pass of the
    same inputs gives; `pin` needs rays (or xyz + z_vals) and no sun_d.  `depth_mode` / `scratch` as for render_pass_into.  Returns the
    workspace."""
    return render_pass_into(spec, params, pin, None, None, out, packed=packed, workspace=workspace, geometry=True,
                            depth_mode=depth_mode, scratch=scratch)


@torch.no_grad()
def relight_pass_into(spec: ModelSpec, params: dict, sun_d: torch.Tensor, t: torch.Tensor, t_s: torch.Tensor | None, out: dict,
                      workspace: torch.Tensor, packed: torch.Tensor | None = None, n_samples: int | None = None,
                      depth_mode: str = "mean", scratch: dict | None = None) -> torch.Tensor:
    """The chunk that `workspace` holds, under another sun: `workspace` is the tensor the BASE pass returned -- the last
    render_pass_into main pass on it, with this spec, these parameters and the same number of rays and samples.  Only what depends on
    the sun runs again (the extras columns, the sun block of the first head layer, the sun-visibility layers, the sky colour, the
    composite: snerf_forward under SNERF_FLAG_RELIGHT); positions, encoding, the trunk, sigma and the other heads are the base
    pass's, and so are the depths.  Every result has the bits of a full pass under `sun_d` (N, 3).  `t` / `t_s` as in the base pass
    (or others: the extras block is rewritten whole).  `out` as for render_pass_into (main-pass keys); N comes from `t`, S from
    `n_samples` or from the shape of a per-sample result tensor in `out`.  Any number of relights may follow one base pass; the
    library refuses a workspace whose last pass was not such a base pass (RuntimeError with its message), but cannot know that the
    caller wrote into the tensor itself.  `depth_mode` / `scratch` as for render_pass_into: the median is that of the relit weights,
    whatever the base pass's mode was.  Returns the workspace."""
    median = _depth_mode_flag("relight_pass_into", depth_mode, out)
    N = t.shape[0]
    S = n_samples
    for k, v in out.items():      # a per-sample result names S: (N, S) or (N, S, c)
        if S is None and k in ("weights", "transparency", "sigmas", "z_vals", "albedo", "sun", "sky", "beta", "beta_semantic") and v.dim() >= 2:
            S = v.shape[1]
    if S is None:
        raise ValueError("relight_pass_into: pass n_samples= (no per-sample result tensor in `out` to take it from)")
    so = _outputs_struct("relight_pass_into", spec, out, N, int(S))
    if workspace is None:
        raise ValueError("relight_pass_into: workspace= must be the tensor the base pass returned")
    pin = PassInputs(sun_d=sun_d)      # (held, with tc / tsc, until the launch is queued: they own the contiguous copies)
    _, _, nbytes, tc, tsc, launch = _forward_setup(spec, pin, t, t_s, _lib.FLAG_RELIGHT | median, n_samples=S)
    if workspace.numel() < nbytes or workspace.device != t.device:
        raise ValueError(f"relight_pass_into: the workspace holds {workspace.numel()} bytes on {workspace.device}, the base pass of "
                         f"{N} x {S} needs {nbytes} on {t.device}")
    held = _bind_median_scratch(so, out, N, int(S), t.device, scratch) if median else None
    if packed is None:
        packed = pack_params(spec, params)
    launch(packed, so, workspace)
    del pin, tc, tsc, held
    return workspace


class _EmbedRows(torch.autograd.Function):
    """rows = table[idx] with the library's deterministic backward (snerf_embedding_rows / snerf_embedding_backward)."""

    @staticmethod
    def forward(ctx, table, idx):
        _check_dev(table, "embedding table")
        tb = table.detach().contiguous()
        ix = idx.contiguous()
        rows = _empty((ix.shape[0], tb.shape[1]), dtype=torch.float32, device=tb.device)
        _lib.call("snerf_embedding_rows", tb, tb.shape[0], tb.shape[1], ix, ix.shape[0], rows)
        ctx.save_for_backward(ix)
        ctx.shape = tuple(tb.shape)
        return rows

    @staticmethod
    def backward(ctx, g):
        (ix,) = ctx.saved_tensors
        grad = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        _lib.call("snerf_embedding_backward", ix, g.contiguous(), ix.shape[0], ctx.shape[1], ctx.shape[0], grad)
        return grad, None


def embed_rows(embedding: torch.nn.Module, idx: torch.Tensor) -> torch.Tensor:
    """models["t"](ts) of the reference renderers (semantic/components/rendering.py:35-46): the rays' rows of an
    nn.Embedding.  torch's embedding backward is a sort + segmented-scatter chain of ~12 launches; here forward and
    backward are one launch each, the backward summed in a fixed order."""
    if idx.dtype != torch.int64:
        idx = idx.long()
    return _EmbedRows.apply(embedding.weight, idx)


def sample_z(rays: torch.Tensor, z_steps: torch.Tensor, u: torch.Tensor | None) -> torch.Tensor:
    """stratified depths (N,S) -- snerf_sample_z"""
    _check_dev(rays, "rays")
    N, S = rays.shape[0], z_steps.shape[0]
    z = _empty((N, S), dtype=torch.float32, device=rays.device)
    _lib.call("snerf_sample_z", rays.contiguous(), z_steps.contiguous(), u.contiguous() if u is not None else None, z, N, S)
    return z


def resample_z(z: torch.Tensor, weights: torch.Tensor, n_importance: int, u: torch.Tensor | None = None, return_fine: bool = False):
    """importance resampling of the depths -- snerf_resample_z (the reference's sample_pdf, framework/components/rendering.py:8-51,
    and the sort of the merged depths): `n_importance` fine samples per ray from the pdf that a proposal pass's `weights` (N, S)
    define over the midpoints of the coarse depths `z` (N, S), merged with `z` -> (N, S + n_importance), non-decreasing along a
    ray.  `u` (N, n_importance) are the uniforms; None = the reference's det=True (a regular grid).  With `return_fine` also the
    fine samples alone, (N, n_importance) in u's order.  One launch on the current stream, no synchronisation; the result
    carries no gradient (sample_pdf's callers detach it)."""
    _check_dev(z, "z")
    _check_dev(weights, "weights")
    Ni = int(n_importance)
    if z.dim() != 2 or tuple(weights.shape) != tuple(z.shape):
        raise ValueError(f"resample_z: z and weights must both be (N, S), got {tuple(z.shape)} and {tuple(weights.shape)}")
    N, S = z.shape
    if u is not None:
        _check_dev(u, "u")
        if tuple(u.shape) != (N, Ni):
            raise ValueError(f"resample_z: u must be (N, n_importance) = {(N, Ni)}, got {tuple(u.shape)}")
    for name, v in (("z", z), ("weights", weights), ("u", u)):
        if v is not None and not v.is_contiguous():
            raise ValueError(f"resample_z: '{name}' must be contiguous")
    z_out = _empty((N, max(S + Ni, 0)), dtype=torch.float32, device=z.device)
    z_fine = _empty((N, max(Ni, 0)), dtype=torch.float32, device=z.device) if return_fine else None
    _lib.call("snerf_resample_z", z.detach(), weights.detach(), u.detach() if u is not None else None, z_out, z_fine, N, S, Ni)
    return (z_out, z_fine) if return_fine else z_out


def ray_distortion(weights: torch.Tensor, z_vals: torch.Tensor, rays: torch.Tensor, per_ray: bool = False, acc: torch.Tensor | None = None):
    """the distortion loss on a pass's weights -- snerf_ray_distortion (include/snerf_hip.h): for
    `weights` (N, S) composited along `z_vals` (N, S) on `rays` (N, >= 8; near and far are columns 6 and 7) ->
    (d_weights_unit, acc[, per_ray]): d L_r / d weights (N, S) of every ray's own value, unscaled; `acc`, four int64 words
    (the library's u64 words: [0] the sum of the rays' values in units of 2^-40, [1] the rays, [2] the bad rays, [3] unused);
    with `per_ray` the rays' values (N,) fp64, NaN for a bad ray.  A given `acc` is accumulated into (shards of one batch), else
    a zeroed one is made.  One launch on the current stream, no synchronisation; nothing here carries a gradient."""
    _check_dev(weights, "weights")
    _check_dev(z_vals, "z_vals")
    _check_dev(rays, "rays")
    if weights.dim() != 2 or tuple(z_vals.shape) != tuple(weights.shape):
        raise ValueError(f"ray_distortion: weights and z_vals must both be (N, S), got {tuple(weights.shape)} and {tuple(z_vals.shape)}")
    N, S = weights.shape
    if rays.dim() != 2 or rays.shape[0] != N or rays.shape[1] < 8:
        raise ValueError(f"ray_distortion: rays must be (N, >= 8) = ({N}, >= 8), got {tuple(rays.shape)}")
    for name, v in (("weights", weights), ("z_vals", z_vals), ("rays", rays), ("acc", acc)):
        if v is not None and not v.is_contiguous():
            raise ValueError(f"ray_distortion: '{name}' must be contiguous")
    if weights.device != z_vals.device or weights.device != rays.device:
        raise ValueError(f"ray_distortion: weights, z_vals and rays must share a device, got {weights.device}, {z_vals.device}, {rays.device}")
    if acc is None:
        acc = torch.zeros(4, dtype=torch.int64, device=weights.device)
    elif not acc.is_cuda or acc.device != weights.device or acc.dtype != torch.int64 or tuple(acc.shape) != (4,):
        raise ValueError(f"ray_distortion: acc must be 4 int64 words on {weights.device}, got {tuple(acc.shape)} {acc.dtype} on {acc.device}")
    d_weights = _empty((N, S), dtype=torch.float32, device=weights.device)
    values = _empty((N,), dtype=torch.float64, device=weights.device) if per_ray else None
    _lib.call("snerf_ray_distortion", weights.detach(), z_vals.detach(), rays.detach(), rays.shape[1], N, S, d_weights, values, acc)
    return (d_weights, acc, values) if per_ray else (d_weights, acc)


_NORMALS_SCRATCH: dict = {}      # (device index, stream id) -> the scratch tensor of density_grad_into, grown as needed


@torch.no_grad()
def density_grad_into(spec: ModelSpec, params: dict, pin: PassInputs, t: torch.Tensor, t_s: torch.Tensor | None = None,
                      coef: torch.Tensor | None = None, out: dict | None = None, want_samples: bool = False,
                      packed: torch.Tensor | None = None) -> dict:
    """coef * d sigma / d xyz of one ray batch -- snerf_density_grad (include/snerf_normals.h): a training forward
    on a leased training workspace, then the backward between a cotangent on sigma and the sample positions alone.  `coef` (N, S) fp32
    weighs the samples; None = the pass's own compositing weights, so that -grad / |grad| is the ray's surface normal.  Returns
    {"grad": (N, 3) fp64, the sum over a ray's samples in normalised scene coordinates; "weights" (N, S); "depth" (N); with
    `want_samples` also "grad_samples" (N, S, 3) fp32}.  `out` may carry preallocated contiguous tensors under those keys (and
    "z_vals" (N, S)), which are then written in place.  The main pass only; the default arithmetic only.  Launches on the current
    stream, no synchronisation."""
    if t is None:
        raise ValueError("density_grad_into: t (N, tau) is required")
    _check_dev(t, "t")
    if coef is not None:
        _check_dev(coef, "coef")
    N, dev = t.shape[0], t.device
    S, d, nbytes, tc, tsc, launch = _forward_setup(spec, pin, t, t_s, _lib.FLAG_TRAIN)
    out = dict(out) if out is not None else {}
    shapes = {"grad": ((N, 3), torch.float64), "weights": ((N, S), torch.float32), "depth": ((N,), torch.float32),
              "grad_samples": ((N, S, 3), torch.float32), "z_vals": ((N, S), torch.float32)}
    for k, v in out.items():
        if k not in shapes:
            raise KeyError(f"density_grad_into: '{k}' is not a result of this pass (have {sorted(shapes)})")
        if not v.is_cuda:
            raise RuntimeError(f"snerf_amd: out['{k}'] must live on the GPU (the HIP path has no CPU fallback)")
        if tuple(v.shape) != shapes[k][0] or v.dtype != shapes[k][1] or not v.is_contiguous():
            raise ValueError(f"density_grad_into: out['{k}'] must be a contiguous {shapes[k][0]} {shapes[k][1]} tensor, got {tuple(v.shape)} {v.dtype}")
    for k in ("grad", "weights", "depth") + (("grad_samples",) if want_samples else ()):
        if k not in out:
            out[k] = _empty(shapes[k][0], dtype=shapes[k][1], device=dev)
    if coef is not None and (tuple(coef.shape) != (N, S) or not coef.is_contiguous()):
        raise ValueError(f"density_grad_into: coef must be a contiguous (N, S) = {(N, S)} tensor, got {tuple(coef.shape)}")
    if packed is None:
        packed = pack_params(spec, params)
    n_scratch = _lib.C.c_size_t(0)
    _lib.check(_lib._invoke("snerf_normals_scratch_bytes", (d, n_scratch), None), "snerf_normals_scratch_bytes")
    with torch.cuda.device(dev):
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
        scratch = _NORMALS_SCRATCH.get(key)
        if scratch is None or scratch.numel() < n_scratch.value:
            scratch = _NORMALS_SCRATCH[key] = _empty(n_scratch.value, dtype=torch.uint8, device=dev)
        lease = lease_workspace(dev, nbytes)
    so = _lib.SnerfOutputs()
    so.weights, so.depth = out["weights"].data_ptr(), out["depth"].data_ptr()
    if "z_vals" in out:
        so.z_vals = out["z_vals"].data_ptr()
    try:
        launch(packed, so, lease.t)
        _lib.call("snerf_density_grad", d, packed, pin.struct(tc, tsc), coef if coef is not None else out["weights"], out["grad"],
                  out.get("grad_samples") if want_samples else None, lease.t, scratch)
    finally:
        lease.release()
    if not want_samples:
        out.pop("grad_samples", None)
    return out

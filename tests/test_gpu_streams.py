"""The stream hand-overs of a training step under forced timing (tests/stream_stall.py; DESIGN.md, 'Streams of a training step').

fused_model_rendering runs the main pass and the solar-correction (sc) pass on two HIP streams, autograd replays each backward on
its forward's stream, both add their gradients into FlatAdam's bucket through an event chain, and TrainLoop gathers the next
batch on a data stream.  At test sizes every kernel is over before the host issues the next, so none of the waits between those
streams can change a bit -- unless a stream is made late on purpose.  Every case here stalls one stream (and, in the `scribble`
cases, overwrites whatever memory a too-early free hands back), then asks for the BITS of the serial run: OVERLAP_SC_PASS off, no
stall -- the path the parity suite holds against the fp64 oracle.  Two contributions add the same in either order, so bit equality
is what ops.py promises; nothing here has a tolerance.  Every stalled case proves, before it synchronises, that its stall was still
running when the host had issued the section under test.

Section 4 pins "every launch of an entry lands on the caller's stream" for the entries a training step calls: with the default
stream stalled, the entry and the copy-out of its results run under a side stream and are complete after side.synchronize() alone."""
import dataclasses

import pytest
import torch

from oracle import snerf_oracle as O
from tests import stream_stall as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(t):
    """a host copy whose equality is bit equality (NaN payloads and signed zeros included)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _assert_same_bits(got: dict, want: dict, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    bad = [k for k in want if got[k].shape != want[k].shape or not torch.equal(got[k], want[k])]
    assert not bad, f"{what}: differs from the serial reference in {bad}"


# ---- 2. the render call, forward and backward --------------------------------------------------------------------------------------
# sub-tile and ragged in the default arithmetic; W = 512 one-plane, where a training pass runs the trunk as one persistent launch
# over tile counters
SHAPES = {"n77-s24-w64": dict(N=77, S=24, W=64, mfma="f16x2"), "n301-s32-w512-f16x1": dict(N=301, S=32, W=512, mfma="f16x1")}
TIMINGS = ("f-none", "a-main-before-call", "b-side-before-call", "c-side-before-sc-backward", "d-main-before-main-backward",
           "e-c-scribble", "e-d-scribble")
_RIGS, _SERIAL = {}, {}


def _rig(shape):
    """one pipeline, optimiser (whose .grad views are the registered sinks) and batch per shape, kept for the module"""
    if shape not in _RIGS:
        from tests.test_gpu_pipeline import _pipeline_for
        from snerf_amd import ops, _lib
        from snerf_amd.framework.components.rendering import z_steps_on
        sh = SHAPES[shape]
        N, S = sh["N"], sh["S"]
        cfg = O.OracleCfg(fc_units=sh["W"], n_samples=S)
        assert cfg.sc_lambda > 0
        pipe, _ = _pipeline_for(cfg, N, 7, mfma_precision=sh["mfma"])
        opt = pipe.configure_optimizers()["optimizer"]
        assert hasattr(opt, "flat_g") and opt.sinks
        spec = pipe.models["coarse"].spec
        assert spec.mfma == sh["mfma"]
        bg = {k: v.to(DEV) for k, v in O.batch_to_torch(O.synthetic_batch(N, S, seed=N + S)).items()}
        # the depths the overlapped path samples for both passes (the same call on the same inputs): handed to the serial run, so
        # that both render on one tensor of depths by construction
        z = ops.sample_z(bg["rays"], z_steps_on(DEV, S), bg["u"])
        d = spec.desc(N, S)
        tau = cfg.t_embedding_tau
        # bytes of every tensor that crosses a stream in the render call: the pack, z, the rows, sun_d (a view of extras), rays; the
        # three sc results (and their cotangents: the same sizes); pg and d_t of the sc pass's backward
        sizes = sorted({4 * _lib.call_size("snerf_packed_floats", d), 4 * N * S, 4 * N * tau, 4 * N * 4, 4 * N * 8,
                        4 * _lib.call_size("snerf_grad_floats", d)})
        torch.cuda.synchronize()
        _RIGS[shape] = dict(pipe=pipe, opt=opt, cfg=cfg, bg=bg, z=z, sizes=sizes, N=N, S=S)
    return _RIGS[shape]


def _render_step(rig, sinks, timing, monkeypatch, given_z=None):
    """zero the bucket, render through fused_model_rendering, the oracle's loss set on the results, backward into every parameter and
    the embedding table (all of them slices of FlatAdam's flat bucket) -> the bits of every result, loss term and the bucket"""
    from snerf_amd import ops, _lib
    from snerf_amd.semantic.components import rendering
    pipe, opt, cfg, bg = rig["pipe"], rig["opt"], rig["cfg"], rig["bg"]
    # the renderer's side stream for this test: one that demonstrably runs beside the main stream (stream_stall.concurrent_streams)
    main, side = torch.cuda.current_stream(DEV), SS.concurrent_streams(DEV)[0]
    monkeypatch.setitem(rendering._SIDE_STREAMS, (DEV.type, DEV.index), side)
    assert rendering._side_stream(DEV) is side
    opt.zero_grad()
    # Every run renders the same batch with the same weights, so a block that comes back from a pool still holds the RIGHT values of
    # the run before: a pass that read it too early would get away with it.  The free blocks of the sizes that cross a stream are
    # therefore filled with NaN first, in both streams' pools.
    for s in (main, side) if given_z is None else ():      # (the serial reference runs as it is: no stall, no scribble)
        SS.scribble(rig["sizes"], s)      # (not held: filled, then free again)
    torch.cuda.synchronize()
    early = []
    if timing.startswith("a-"):
        early.append(SS.stall(main))      # the side stream must wait for the pack, z and the rows
    if timing.startswith("b-"):
        early.append(SS.stall(side))      # the loss on the main stream must wait for the sc results
    opts = {"perturb_rand": bg["u"], "return_z_vals": True}
    if given_z is not None:
        opts["given_z_vals"] = given_z
    res = pipe.renderer.render_rays(pipe.models, bg["rays"], bg["extras"], render_options=opts)
    # O.training_losses at an epoch past first_beta_epoch, in its order, term group by term group: the semantic loss indexes with a
    # boolean mask, the one host synchronisation of the set, and the guard of a / b has to be read before it (the colour and
    # solar-correction terms, which read the sc results on the main stream, are issued by then)
    ld = O.satnerf_loss(res, bg["rgbs"], cfg)
    for ev in early:
        SS.still_running(ev, "the render call and the loss terms that read the sc results")
    ld.update(O.semantic_loss(res, bg["semantic"], bg["mask"], cfg))
    total = O.total_loss(ld)

    late, cot, real_call = [], [], _lib.call
    stall_sc = "c-" in timing
    if stall_sc or "d-" in timing:
        target = side if stall_sc else main

        def call(name, *args, **kw):
            if name == "snerf_backward" and not late and bool(args[0].flags & _lib.FLAG_SC_PASS) == stall_sc:
                assert torch.cuda.current_stream(DEV) == target, "autograd did not replay the pass's backward on its forward's stream"
                late.append(SS.stall(target))
                cot.append(args[3].sun)      # the address of the sc pass's one cotangent (the loss made it on the main stream)
            return real_call(name, *args, **kw)
        monkeypatch.setattr(_lib, "call", call)
    if sinks:
        with ops.accumulate_into_sinks():
            total.backward()
        ops.wait_grad_sinks()
    else:
        total.backward()
    monkeypatch.setattr(_lib, "call", real_call)
    held = []
    if timing.startswith("e-"):
        held += SS.scribble(rig["sizes"], main)      # as soon as backward() has returned on the host
        if stall_sc and cot[0]:
            # a measurement, not a check: with the side stream still stalled in front of the read, did the main stream's pool hand
            # the cotangent's block out again?  (It may: by then the main stream waits for the side stream's backward.)
            print(f"\n[{timing}, {'sinks' if sinks else 'autograd'}] the sc pass's cotangent block was handed out again before the side "
                  f"stream had read it: {any(t.data_ptr() == cot[0] for t in held)}")
    # (copies queued on the main stream behind everything above: what a consumer on that stream sees)
    got = {k: v.detach().clone() for k, v in res.items()}
    got.update({"loss/" + k: v.detach().clone() for k, v in ld.items()})
    got["flat_g"] = opt.flat_g.clone()
    del res, ld, total      # the graph dies: the pack, z, the rows and the cotangents the passes held go back to their pools
    if timing.startswith("e-"):
        held += SS.scribble(rig["sizes"], main)
    if stall_sc or "d-" in timing:
        assert len(late) == 1, "the stalled snerf_backward was never called"
        SS.still_running(late[0], "backward(), the wait for the sinks and the scribbles")
    torch.cuda.synchronize()
    del held
    return {k: _bits(v) for k, v in got.items()}


def _serial(shape, sinks):
    """the reference: both passes on one stream, no stall, no scribble; computed once per (shape, sink path) and left unchanged"""
    key = (shape, sinks)
    if key not in _SERIAL:
        from snerf_amd.semantic.components import rendering
        rig = _rig(shape)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(rendering, "OVERLAP_SC_PASS", False)      # (read at import: the env var alone would change nothing)
            ref = _render_step(rig, sinks, "f-none", mp, given_z=rig["z"])
            again = _render_step(rig, sinks, "f-none", mp, given_z=rig["z"])
        _assert_same_bits(again, ref, "the serial run is not reproducible")
        assert all(bool(torch.isfinite(v.view(torch.float32)).all()) for k, v in ref.items() if v.dtype == torch.int32), "reference has non-finite values"
        assert bool((ref["flat_g"] != 0).any())
        _SERIAL[key] = ref
    return _SERIAL[key]


@pytest.mark.parametrize("timing", TIMINGS)
@pytest.mark.parametrize("sinks", (False, True), ids=("autograd-accumulates", "sinks"))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_overlapped_render_step_has_the_bits_of_the_serial_one(shape, sinks, timing, monkeypatch):
    """Timings a-f of DESIGN.md 'Streams of a training step': whichever stream is late, and whatever the allocator hands out in the
    meantime, every result, every loss term and the whole gradient bucket (every parameter and the embedding table) of the
    overlapped render step equal the serial reference bit for bit; the depths the overlapped path samples are the reference's."""
    from snerf_amd.semantic.components import rendering
    assert rendering.OVERLAP_SC_PASS, "the overlap is off (SNERF_OVERLAP_SC=0): nothing to test"
    want = _serial(shape, sinks)
    got = _render_step(_rig(shape), sinks, timing, monkeypatch)
    _assert_same_bits(got, want, f"{shape} / {'sinks' if sinks else 'autograd'} / {timing}")


# ---- 3. the loop -------------------------------------------------------------------------------------------------------------------
_LOOP_SERIAL = {}


def _loop_trajectory(mode, monkeypatch):
    """the step order of test_trainloop_host_side_switches_do_not_change_the_trajectory (consecutive steps over an epoch boundary,
    then a jump in the step index) -> (bits of every step's loss, bits of the final weights)"""
    from tests.test_gpu_optim_ckpt import _loop
    from snerf_amd import _lib
    from snerf_amd.semantic.components import rendering
    loop = _loop(seed=11)
    spe = loop.steps_per_epoch
    order = list(range(0, spe + 2)) + [3 * spe + 1, 3 * spe + 2]
    # three streams that demonstrably run beside each other (stream_stall.concurrent_streams): compute, the sc pass's, the batches'
    main, (side, data) = torch.cuda.current_stream(DEV), SS.concurrent_streams(DEV)
    monkeypatch.setitem(rendering._SIDE_STREAMS, (DEV.type, DEV.index), side)
    assert loop.prefetch and loop._next is None
    loop._data_stream = data
    per_step = []      # the stall event(s) of the step being issued

    if mode == "data-stream":
        batch_ev, issue, take = {}, loop._issue_batch, loop._take_batch

        def stalled_issue(step):
            batch_ev[step] = SS.stall(loop._data_stream, SS.LOOP_STALL_S)
            return issue(step)

        def checked_take(step):
            batch = take(step)
            # the stall in front of this batch's gather is still running: ev.query() was False and the compute stream was told to wait
            SS.still_running(batch_ev.pop(step), f"_take_batch({step})")
            return batch
        loop._issue_batch, loop._take_batch = stalled_issue, checked_take
    if mode == "side-before-sc-backward":
        real_call, opt_step = _lib.call, loop.optimizer.step
        sizes = _loop_sizes(loop)

        def call(name, *args, **kw):
            if name == "snerf_backward" and args[0].flags & _lib.FLAG_SC_PASS:
                assert torch.cuda.current_stream(DEV) == side
                per_step.append(SS.stall(side, SS.LOOP_STALL_S))
            return real_call(name, *args, **kw)

        def scribbled_step(*a, **k):
            held.extend(SS.scribble(sizes, main))
            return opt_step(*a, **k)
        monkeypatch.setattr(_lib, "call", call)
        loop.optimizer.step = scribbled_step
    losses, held = [], []      # (the scribbles are held until the final synchronise)
    for s in order:
        torch.manual_seed(500 + s)
        del per_step[:]
        if mode == "main-before-step":
            per_step.append(SS.stall(main, SS.LOOP_STALL_S))
        losses.append(loop.step(s)["loss"].detach())
        assert len(per_step) == (0 if mode in (None, "data-stream") else 1), (mode, s, len(per_step))
        for ev in per_step:
            SS.still_running(ev, f"step {s}")
    torch.cuda.synchronize()
    if mode == "data-stream":
        # never taken: the batch prefetched in front of the jump, and the one behind the last step
        assert sorted(batch_ev) == [spe + 2, 3 * spe + 3], sorted(batch_ev)
        assert len(held) == 0
    if mode == "side-before-sc-backward":
        assert len(held) == 4 * len(sizes) * len(order)
    return _bits(torch.stack(losses)), [_bits(p) for p in loop.pipeline.parameters()]


def _loop_sizes(loop):
    """byte sizes of what crosses a stream in a step of `loop` (as in _rig)"""
    from snerf_amd import _lib
    pc = loop.cfgs.pipeline
    spec = loop.pipeline.models["coarse"].spec
    N, S = loop.global_batch, pc.n_samples
    d = spec.desc(N, S)
    return sorted({4 * _lib.call_size("snerf_packed_floats", d), 4 * N * S, 4 * N * pc.t_embedding_tau, 4 * N * 4, 4 * N * 8,
                   4 * _lib.call_size("snerf_grad_floats", d)})


@pytest.mark.parametrize("mode", ("data-stream", "side-before-sc-backward", "main-before-step"))
def test_trainloop_under_stalls_follows_the_serial_trajectory(mode, monkeypatch):
    """TrainLoop.step with (data-stream) every batch gather behind a stall on the data stream -- _take_batch finds the event
    incomplete and queues the wait; (side-before-sc-backward) the side stream stalled in front of every sc backward and the main
    stream's pools scribbled right before optimizer.step(); (main-before-step) the main stream stalled in front of every step: the
    losses of all steps and the final weights are those of the serial loop (OVERLAP_SC_PASS off, no stall), bit for bit."""
    from snerf_amd.semantic.components import rendering
    assert rendering.OVERLAP_SC_PASS
    if "ref" not in _LOOP_SERIAL:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(rendering, "OVERLAP_SC_PASS", False)
            _LOOP_SERIAL["ref"] = _loop_trajectory(None, mp)
    want_l, want_w = _LOOP_SERIAL["ref"]
    assert bool(torch.isfinite(want_l.view(torch.float32)).all())
    got_l, got_w = _loop_trajectory(mode, monkeypatch)
    assert torch.equal(got_l, want_l), (mode, got_l.view(torch.float32).tolist(), want_l.view(torch.float32).tolist())
    assert len(got_w) == len(want_w) and all(torch.equal(a, b) for a, b in zip(got_w, want_w)), mode


# ---- 4. every launch of a training-step entry lands on the caller's stream ---------------------------------------------------------
def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _lands_on_the_callers_stream(setup, launch, outputs):
    """The pattern of test_call_lands_on_the_current_stream.  setup() -> fresh buffers (everything the entry consumes already issued
    on the default stream); launch(bufs) issues the entry; outputs(bufs) -> the tensors it writes.  Once unstalled on the default
    stream for the wanted bits; then with the default stream stalled, the entry and the copies to pinned memory under a side
    stream: complete after side.synchronize() alone, while the default stream's stall is still running."""
    ref = setup()
    launch(ref)
    torch.cuda.synchronize()
    want = [_bits(t) for t in outputs(ref)]
    bufs = setup()
    outs = outputs(bufs)
    host = [torch.zeros(t.shape, dtype=t.dtype).pin_memory() for t in outs]
    side = SS.concurrent_streams(DEV)[0]      # (not torch.cuda.Stream() as it comes: one in four shares the default stream's hardware queue)
    torch.cuda.synchronize()
    ev = SS.stall(torch.cuda.default_stream(DEV))
    with torch.cuda.stream(side):
        launch(bufs)
        for h, t in zip(host, outs):
            h.copy_(t, non_blocking=True)
    side.synchronize()
    same = [torch.equal(_bits(h), w) for h, w in zip(host, want)]
    running = not ev.query()
    torch.cuda.synchronize()
    assert running, "stall too short: the default stream was idle again at the moment of comparison"
    assert all(same), f"results {[i for i, s in enumerate(same) if not s]} were not complete (or not right) after the side stream alone"
    assert len(want) > 0 and all(w.numel() > 0 for w in want)


_CASES = {}
N4, S4 = 77, 24


def _case(width):
    """spec, parameters, pack and one batch at N = 77, S = 24: W = 64 in the default arithmetic, W = 512 one-plane"""
    if width not in _CASES:
        from tests.test_gpu_kernels import _spec, _gpu_params
        from snerf_amd import ops
        W = 64 if width == "w64" else 512
        cfg = O.OracleCfg(fc_units=W, n_samples=S4)
        spec = _spec(cfg) if W == 64 else dataclasses.replace(_spec(cfg), mfma="f16x1")
        gp = _gpu_params(O.init_params_numpy(cfg, 3), DEV)
        b = {k: v.to(DEV) for k, v in O.batch_to_torch(O.synthetic_batch(N4, S4, seed=41)).items()}
        table = torch.from_numpy(O.init_embedding_numpy(cfg, 3)).to(DEV)
        idx = b["extras"][:, 3].long().contiguous()
        zs = torch.linspace(0, 1, S4).to(DEV)
        c = dict(cfg=cfg, spec=spec, gp=gp, b=b, table=table, idx=idx, zs=zs, t=table[idx].contiguous(),
                 packed=ops.pack_params(spec, gp), z=ops.sample_z(b["rays"], zs, b["u"]))
        torch.cuda.synchronize()
        _CASES[width] = c
    return _CASES[width]


def _forward_bufs(c, flags):
    """NaN-filled results (labels -1), inputs struct, workspace and the launch of snerf_forward under `flags`"""
    from snerf_amd import ops, _lib
    spec, b = c["spec"], c["b"]
    sc, geom = bool(flags & _lib.FLAG_SC_PASS), bool(flags & _lib.FLAG_GEOMETRY)
    keys = list(ops.GEOMETRY_KEYS) if geom else ops.output_keys(spec, sc) + ([] if sc else ["semantic_label", "z_vals"])
    out = {}
    for k in keys:
        if k == "semantic_label":
            out[k] = torch.full((N4,), -1, dtype=torch.int64, device=DEV)
        else:
            out[k] = _nan(*((N4, S4) if k == "z_vals" else ops._OUT_SHAPES[k](N4, S4, spec.n_classes)))
    sun = b["extras"][:, :3]
    if geom:
        pin, t = ops.PassInputs(rays=b["rays"], z_steps=c["zs"], u=b["u"]), None
    elif sc:
        pin, t = ops.PassInputs(sun_d=sun, rays=b["rays"], z_vals=c["z"]), c["t"]
    else:
        pin, t = ops.PassInputs(sun_d=sun, rays=b["rays"], z_steps=c["zs"], u=b["u"]), c["t"]
    S, d, nbytes, tc, _, launch = ops._forward_setup(spec, pin, t, None, flags)
    assert S == S4
    so = ops._outputs_struct("test", spec, out, N4, S4, sc_pass=sc, geometry=geom)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return dict(out=out, so=so, ws=ws, d=d, nbytes=nbytes, pin=pin, tc=tc, launch=lambda: launch(c["packed"], so, ws))


def test_pack_params_lands_on_the_callers_stream():
    from snerf_amd import ops, _lib
    c = _case("w64")
    d = c["spec"].desc(1, 1)
    n = _lib.call_size("snerf_packed_floats", d)
    ps = ops.params_struct(c["spec"], c["gp"])
    _lands_on_the_callers_stream(lambda: {"packed": _nan(n)},
                                 lambda bufs: _lib.call("snerf_pack_params", d, ps, bufs["packed"]),
                                 lambda bufs: [bufs["packed"]])


def _fwd_flags():
    from snerf_amd import _lib
    return {"train": _lib.FLAG_TRAIN, "train-sc": _lib.FLAG_TRAIN | _lib.FLAG_SC_PASS, "inference": 0,
            "geometry-median": _lib.FLAG_GEOMETRY | _lib.FLAG_DEPTH_MEDIAN}


@pytest.mark.parametrize("mode", ("train", "train-sc", "inference", "geometry-median"))
@pytest.mark.parametrize("width", ("w64", "w512-f16x1"))
def test_forward_lands_on_the_callers_stream(width, mode):
    """snerf_forward: every launch and asynchronous copy of the pass, for the training main and sc pass, the inference pass and the
    geometry pass with the median launch behind it"""
    c = _case(width)
    flags = _fwd_flags()[mode]
    _lands_on_the_callers_stream(lambda: _forward_bufs(c, flags), lambda bufs: bufs["launch"](), lambda bufs: list(bufs["out"].values()))


@pytest.mark.parametrize("mode", ("full", "embed-grad", "sc-full"))
@pytest.mark.parametrize("width", ("w64", "w512-f16x1"))
def test_backward_lands_on_the_callers_stream(width, mode):
    """snerf_backward (the full backward of the main and of the sc pass, and the embedding-only one) behind a training forward that
    ran on the default stream: the packed gradients and d_t"""
    from snerf_amd import _lib
    c = _case(width)
    sc = mode == "sc-full"
    g = torch.Generator().manual_seed(5)

    def setup():
        f = _forward_bufs(c, _lib.FLAG_TRAIN | (_lib.FLAG_SC_PASS if sc else 0))
        f["launch"]()
        go, cot = _lib.SnerfOutGrads(), []
        for k, v in f["out"].items():
            if k in _lib.GRAD_FIELDS:
                cot.append((torch.randn(v.shape, generator=g) * 0.1).to(DEV))
                setattr(go, k, cot[-1].data_ptr())
        d = _lib.SnerfDesc.from_buffer_copy(f["d"])
        if mode == "embed-grad":
            d.flags |= _lib.FLAG_EMBED_GRAD
        pg = None if mode == "embed-grad" else torch.zeros(_lib.call_size("snerf_grad_floats", f["d"]), device=DEV)
        f.update(go=go, cot=cot, desc=d, pg=pg, d_t=_nan(*c["t"].shape))
        return f

    def launch(f):
        _lib.call("snerf_backward", f["desc"], c["packed"], f["pin"].struct(f["tc"], None), f["go"], f["pg"], f["d_t"], None,
                  f["ws"], f["nbytes"])

    # the generator advances from setup to setup: both setups must see the same cotangents
    state = g.get_state()

    def same_setup():
        g.set_state(state)
        return setup()
    _lands_on_the_callers_stream(same_setup, launch, lambda f: [f["d_t"]] + ([f["pg"]] if f["pg"] is not None else []))


@pytest.mark.parametrize("accumulate", (False, True), ids=("overwrite", "accumulate"))
def test_unpack_grads_lands_on_the_callers_stream(accumulate):
    from snerf_amd import ops, _lib
    c = _case("w64")
    spec = c["spec"]
    d = spec.desc(1, 1)
    pg = torch.randn(_lib.call_size("snerf_grad_floats", spec.desc(N4, S4)), generator=torch.Generator().manual_seed(8)).to(DEV)      # (sized as ops._RenderPass.backward sizes it)

    def setup():
        grads = {n: (torch.full_like(c["gp"][n], 0.5) if accumulate else _nan(*c["gp"][n].shape)) for n in spec.param_names()}
        return {"grads": grads, "ps": ops.params_struct(spec, grads)}
    _lands_on_the_callers_stream(setup, lambda bufs: _lib.call("snerf_unpack_grads", d, pg, bufs["ps"], int(accumulate)),
                                 lambda bufs: list(bufs["grads"].values()))


def _loss_problem(**cfg_fields):
    """one SnerfLossCfg / SnerfLossIn over random rendered tensors (N = 77, S = 24, five classes) and a runner that issues
    snerf_loss_partial + snerf_loss_finish into fresh NaN-filled totals, terms and gradients"""
    from snerf_amd import _lib
    C = 5
    g = torch.Generator().manual_seed(19)
    t = {"rgb": torch.rand(N4, 3, generator=g), "weights": torch.rand(N4, S4, generator=g) * 0.1,
         "beta": torch.rand(N4, S4, 1, generator=g) + 0.01, "semantic_logits": torch.rand(N4, C, generator=g) * 3,
         "sun_sc": torch.rand(N4, S4, 1, generator=g), "transparency_sc": torch.rand(N4, S4, generator=g),
         "weights_sc": torch.rand(N4, S4, generator=g) * 0.1, "depth": torch.rand(N4, generator=g),
         "gt_rgb": torch.rand(N4, 3, generator=g), "gt_depth": torch.rand(N4, generator=g), "depth_weights": torch.rand(N4, generator=g)}
    t = {k: v.to(DEV) for k, v in t.items()}
    labels = torch.randint(0, C, (N4,), generator=g)
    labels[::6] = 4
    t["labels"] = labels.to(DEV)
    t["mask"] = (torch.rand(N4, generator=g) > 0.3).to(torch.uint8).to(DEV)
    fields = dict(n_rays=N4, n_samples=S4, n_classes=C, color_mode=2, has_sc=1, sem_mode=2, ignore_index=4, use_sbeta=0,
                  detach_beta_for_s=0, car_reg=1, car_label=4, has_depth=1, sc_lambda=0.05, lambda_s=0.04, lambda_c=0.1, ds_lambda=1000.0)
    fields.update(cfg_fields)
    cfg = _lib.SnerfLossCfg(**fields)
    li = _lib.SnerfLossIn()
    for k, v in t.items():
        setattr(li, k, v.data_ptr())      # (beta_semantic stays NULL)
    wsb = _lib.call_size("snerf_loss_workspace_bytes", cfg)

    def setup():
        grads = {k: _nan(*t[k].shape) for k in ("rgb", "weights", "beta", "semantic_logits", "sun_sc", "depth")}
        lg = _lib.SnerfLossGrads()
        for k, v in grads.items():
            setattr(lg, k, v.data_ptr())
        return {"grads": grads, "lg": lg, "totals": _nan(_lib.LOSS_NTOT), "terms": _nan(8), "ws": torch.empty(wsb, dtype=torch.uint8, device=DEV)}

    def launch(bufs):
        _lib.call("snerf_loss_partial", cfg, li, bufs["totals"], bufs["ws"], wsb)
        _lib.call("snerf_loss_finish", cfg, li, bufs["totals"], float(N4), 1.0, bufs["terms"], bufs["lg"])

    def outputs(bufs):
        return [bufs["totals"], bufs["terms"]] + list(bufs["grads"].values())
    return t, setup, launch, outputs


def test_loss_partial_and_finish_land_on_the_callers_stream():
    _, setup, launch, outputs = _loss_problem()
    _lands_on_the_callers_stream(setup, launch, outputs)


def test_adam_step_lands_on_the_callers_stream():
    from snerf_amd import _lib
    n = 4 * 1028 + 4
    g = torch.Generator().manual_seed(2)
    p0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    m0, v0 = torch.randn(n, generator=g) * 1e-3, torch.rand(n, generator=g) * 1e-4

    def setup():
        return {k: v.to(DEV) for k, v in (("p", p0), ("g", g0), ("m", m0), ("v", v0))}
    _lands_on_the_callers_stream(setup, lambda b: _lib.call("snerf_adam_step", b["p"], b["g"], b["m"], b["v"], n, 5e-4, 0.9, 0.999, 1e-8, 3, 1.0),
                                 lambda b: [b["p"], b["m"], b["v"]])


def test_embedding_rows_and_backward_land_on_the_callers_stream():
    from snerf_amd import _lib
    c = _case("w64")
    table, idx = c["table"], c["idx"]
    V, tau = table.shape
    _lands_on_the_callers_stream(lambda: {"rows": _nan(N4, tau)},
                                 lambda b: _lib.call("snerf_embedding_rows", table, V, tau, idx, N4, b["rows"]),
                                 lambda b: [b["rows"]])
    d_rows = torch.randn(N4, tau, generator=torch.Generator().manual_seed(4)).to(DEV)
    _lands_on_the_callers_stream(lambda: {"grad": torch.zeros(V, tau, device=DEV)},      # (the entry adds into grad_table)
                                 lambda b: _lib.call("snerf_embedding_backward", idx, d_rows, N4, tau, V, b["grad"]),
                                 lambda b: [b["grad"]])


def test_resample_z_lands_on_the_callers_stream():
    from snerf_amd import _lib
    c = _case("w64")
    Ni = 16
    g = torch.Generator().manual_seed(6)
    w = (torch.rand(N4, S4, generator=g) * 0.1).to(DEV)
    u = torch.rand(N4, Ni, generator=g).to(DEV)
    _lands_on_the_callers_stream(lambda: {"z_out": _nan(N4, S4 + Ni), "z_fine": _nan(N4, Ni)},
                                 lambda b: _lib.call("snerf_resample_z", c["z"], w, u, b["z_out"], b["z_fine"], N4, S4, Ni),
                                 lambda b: [b["z_out"], b["z_fine"]])


def test_ray_distortion_lands_on_the_callers_stream():
    from snerf_amd import _lib
    c = _case("w64")
    rays = c["b"]["rays"]
    w = (torch.rand(N4, S4, generator=torch.Generator().manual_seed(7)) * 0.1).to(DEV)
    _lands_on_the_callers_stream(lambda: {"d_w": _nan(N4, S4), "values": _nan(N4, dtype=torch.float64), "acc": torch.zeros(4, dtype=torch.int64, device=DEV)},
                                 lambda b: _lib.call("snerf_ray_distortion", w, c["z"], rays, rays.shape[1], N4, S4, b["d_w"], b["values"], b["acc"]),
                                 lambda b: [b["d_w"], b["values"], b["acc"]])


# ---- the loss entries with use_sbeta set and no beta_semantic ----------------------------------------------------------------------
def test_loss_reads_beta_semantic_only_for_the_uncertainty_loss():
    """Raw ABI: use_sbeta = 1 with sem_mode = 1 (plain CE) and color_mode = 2 passes check_loss without a beta_semantic pointer, and
    the kernels must not read one: the sum over w * beta_semantic feeds the uncertainty CE (sem_mode = 2) alone.  With NULL
    beta_semantic that configuration gives the bits of use_sbeta = 0 -- totals, terms and every gradient.  (Python never builds this
    configuration: loss_ops.fused_loss hands beta_semantic over only with sem_mode = 2.)"""
    res = {}
    for sbeta in (0, 1):
        t, setup, launch, outputs = _loss_problem(sem_mode=1, use_sbeta=sbeta, car_reg=0)
        bufs = setup()
        launch(bufs)
        torch.cuda.synchronize()
        res[sbeta] = [_bits(x) for x in outputs(bufs)]
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    terms = res[1][1].view(torch.float32)
    assert bool(torch.isfinite(terms).all()) and float(terms[4]) != 0.0 and float(terms[0]) != 0.0

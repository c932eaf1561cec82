"""The device-resident samplers of a denoiser module (``sample_euler_fused``, ``sample_dopri5_device``, ``sample_sde_device``) and the
ONE place that knows when a captured sampler step may be replayed.

Every sampler copies its conditioning into buffers this object owns (``resident``), captures one step into a HIP graph
(``transport.odeint.capture_step``) and holds it, with its state buffers, for the next call: a ``HeldStep`` per sampler kind, found
again through ``signature`` -- everything the captured launches have baked in by address, bound to the generation of the weight pack
they read.  ``DiT._prepare`` calls ``drop()`` whenever it builds a new pack: a held step is never replayed against another pack than the
one it was captured for.  What differs between the samplers is their step body, written once each below.
"""
from __future__ import annotations

import ctypes
import dataclasses

import torch

from .. import dit_ops as ops
from ..transport.odeint import _initial_step, capture_step

KINDS = ("euler", "dopri5", "sde")


@dataclasses.dataclass
class HeldStep:
    """a captured sampler step and what it runs on"""
    bufs: dict                  # the state buffers of the kind, by name: rewritten per call, their addresses are baked into the graph
    sig: tuple | None = None    # DeviceSamplers.signature() at capture time; None: not to be found again
    graph: object = None        # torch.cuda.CUDAGraph of one step
    keep: tuple = ()            # ctypes blocks and context tensors the captured launches point into


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _velocity_step(cfg_scale, cfg, dst):      # an evaluation whose guided velocity leaves through the final-layer kernel into ``dst``
    return ops.GaDitSamplerStep(float(cfg_scale), 1 if cfg else 0, None, None, None, 0, None, dst.data_ptr())


class DeviceSamplers:
    def __init__(self, model):
        self.model = model
        self.generation = 0     # of the model's weight pack: moved by drop()
        self._held = dict.fromkeys(KINDS)
        self._resident = {}

    # -- the held steps -------------------------------------------------------------------------------------------------
    def held(self, kind):
        """the HeldStep of ``kind``, or None"""
        return self._held[kind]

    def lookup(self, kind, sig):
        """the step of ``kind`` an earlier call captured against exactly ``sig``, or None"""
        rec = self._held[kind]
        return rec if sig is not None and rec is not None and rec.sig == sig else None

    def store(self, kind, rec):
        self._held[kind] = rec

    def drop(self):
        """The weight pack changed: release every captured step with its buffers, and bind later signatures to the new pack."""
        self.generation += 1
        self._held = dict.fromkeys(KINDS)

    def stamp(self, baked_in):
        """a signature: what a captured step has baked in, bound to the current pack"""
        return (self.generation,) + tuple(baked_in)

    def resident(self, context):
        """The conditioning of a sampling call copied into buffers this object owns (one set per shape): every evaluation of the call --
        and the captured sampler step, which has their addresses baked in -- reads these, so the step captured for one sample is
        replayed for the next one (capturing ~1 750 launches costs ~10 ms per call)."""
        m, out = self.model, {}
        for name, t in context.items():
            want = torch.float32 if name in (m._vec_key, "fps-xyz") else t.dtype
            buf = self._resident.get(name)
            if buf is None or buf.shape != t.shape or buf.dtype != want or buf.device != t.device:
                buf = torch.empty(t.shape, dtype=want, device=t.device)
            buf.copy_(t.detach())
            out[name] = buf
        self._resident = out
        return out

    def signature(self, context, shape, n, cfg, cfg_scale, key=()):
        """What a captured sampler step has baked in besides its own buffers: the model's workspace, the K / V projections of the
        conditioning tokens (refreshed here, in place when the shapes are those of the previous call), the number of batch items
        that skip the cross-attention, the resident conditioning vectors -- all by address -- and, through ``stamp``, the weight pack.
        ``key``: what else the sampler kind captured differently for.  None: nothing to replay against yet."""
        m = self.model
        B, L, _ = shape
        tok = context[m._ctx_key]
        pack = m._prepare(tok.device)      # (a new pack drops the held steps and moves the generation)
        ck, cvt, ca_batch = m._context_kv(pack, tok)
        if pack.get("ws") is None or pack["ws_key"] != (B, L, tok.shape[1]):
            return None
        sig = [key, tuple(shape), n, bool(cfg), float(cfg_scale), pack["ws"].data_ptr(), ck.data_ptr(), cvt.data_ptr(), ca_batch]
        vec = context[m._vec_key]
        if m.pooled_once and vec.dtype == torch.float32 and vec.is_contiguous():
            sig.append(m._pooled(pack, vec).data_ptr())     # (refreshed in place for this call's vector)
        for name in (m._vec_key,) + (("fps-xyz",) if m._stage2 else ()):
            t = context[name]
            if t.dtype != torch.float32 or not t.is_contiguous():
                return None   # (forward() would hand the kernels a temporary copy)
            sig.append((t.data_ptr(), tuple(t.shape)))
        return self.stamp(sig)

    def _need_velocity(self, what):
        if self.model.out_channels != self.model.in_channels:
            raise ValueError(f"the {what} needs a velocity of the state's shape (learn_sigma=False)")

    def _begin(self, kind, context, *sig_args):
        """what every sampler starts with: residency, and the step held for this call if there is one"""
        context = self.resident(context)
        return context, self.lookup(kind, self.signature(context, *sig_args))

    def _hold(self, kind, rec, graph, keep, context, *sig_args):
        """what every sampler does after its capture: the signature exists now that the first evaluations have sized the workspace and
        cached the K / V; the step is kept for the replays in flight -- and for later calls on the same conditioning"""
        rec.graph, rec.keep = graph, tuple(keep) + tuple(context.values())
        rec.sig = self.signature(context, *sig_args)
        self.store(kind, rec)

    # -- the three step bodies ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def euler(self, y0, t_grid, context, cfg_scale=1.0, cfg=True):
        """The reference's fixed-grid Euler sampling loop (transport/integrators.py:100-119 with method "euler":
        y_{k+1} = y_k + (t_{k+1} - t_k) f(t_k, y_k), all grid states returned) with the whole step on the device: the
        function evaluation, the CFG combine of ``forward_with_cfg`` and the state update leave through the final-layer
        kernel (GaDitSamplerStep), a one-thread kernel moves the step counter / time / step size on, and one step is
        captured into a HIP graph and replayed -- nothing but this library's kernels between two steps, no host
        synchronisation.  Bit-identical to the eager loop over ``forward_with_cfg`` / ``forward_cond``."""
        self._need_velocity("fused sampler step")
        m, dev = self.model, y0.device
        tt = [float(v) for v in t_grid]
        n = len(tt)
        B = y0.shape[0]
        sig_args = (tuple(y0.shape), n, cfg, cfg_scale)
        context, rec = self._begin("euler", context, *sig_args)
        if rec is None:
            f32 = dict(dtype=torch.float32, device=dev)
            rec = HeldStep({"y": torch.empty(tuple(y0.shape), **f32), "out": torch.empty((n,) + tuple(y0.shape), **f32),
                            "t_arr": torch.empty(n - 1, **f32), "dt_arr": torch.empty(n - 1, **f32), "tvec": torch.empty(B, **f32),
                            "counter": torch.zeros(1, dtype=torch.int32, device=dev), "dt": torch.empty(1, **f32)})
        y, out, t_arr, dt_arr, counter, tvec, dt = (rec.bufs[q] for q in ("y", "out", "t_arr", "dt_arr", "counter", "tvec", "dt"))
        out[0].copy_(y0.detach().float())
        if n < 2:
            return out
        t_arr.copy_(torch.tensor(tt[:-1], dtype=torch.float32))
        dt_arr.copy_(torch.tensor([b - a for a, b in zip(tt[:-1], tt[1:])], dtype=torch.float32))

        def reset():
            y.copy_(out[0])
            counter.zero_()
            tvec.fill_(tt[0])
            dt.copy_(dt_arr[0:1])

        if rec.graph is None:
            step = ops.GaDitSamplerStep(float(cfg_scale), 1 if cfg else 0, dt.data_ptr(), y.data_ptr(), out.data_ptr(),
                                        y.numel(), counter.data_ptr(), None)

            def one_step():
                m.forward(y, tvec, context, _step=step)
                ops.check(ops.lib().ga_dit_sampler_advance(counter.data_ptr(), t_arr.data_ptr(), dt_arr.data_ptr(), n - 1,
                                                           tvec.data_ptr(), B, dt.data_ptr(), _stream(dev)), "ga_dit_sampler_advance")

            self._hold("euler", rec, capture_step(one_step, reset, dev), (step,), context, *sig_args)
        else:
            reset()
        for _ in range(n - 1):
            rec.graph.replay()
        return out.clone() if rec.sig is not None else out

    @torch.no_grad()
    def dopri5(self, y0, t_grid, context, cfg_scale=1.0, cfg=True, atol=1e-6, rtol=1e-3, stats=None, max_steps=1 << 16):
        """The reference's DEFAULT sampler -- torchdiffeq's dopri5 behind ``ode.sample`` (transport/integrators.py:100-119,
        flow_matching_trainer.py:715) -- with the adaptive loop on the device (csrc/ode_dopri5.hip): one attempted step = six
        (stage input, function evaluation with the guided velocity leaving through the final-layer kernel) pairs, the error norm, a
        one-thread controller and a predicated accept kernel with the dense output, captured into ONE HIP graph and replayed; time,
        step size, decisions and counters live in a device block and the host only reads the ``done`` word after a replay.  Same
        decisions as ``transport/odeint.py`` / ``oracle/ode.py`` (the initial step size is chosen on the host as there: two
        evaluations).  Returns the states at every requested time."""
        self._need_velocity("device-resident dopri5")
        m, dev = self.model, y0.device
        tt = [float(v) for v in t_grid]
        ng = len(tt)
        Lib = ops.lib()
        B, n = y0.shape[0], y0.numel()
        sig_args = (tuple(y0.shape), ng, cfg, cfg_scale)
        context, rec = self._begin("dopri5", context, *sig_args)
        if rec is None:
            y = torch.empty(tuple(y0.shape), dtype=torch.float32, device=dev)
            rec = HeldStep({"y": y, "out": torch.empty((ng,) + tuple(y.shape), dtype=torch.float32, device=dev),
                            "k": [torch.empty_like(y) for _ in range(7)], "ystage": torch.empty_like(y),
                            "tvec": torch.empty(B, dtype=torch.float32, device=dev),
                            "ctl": torch.zeros(ops.GA_ODE_CTL_ALLOC, dtype=torch.float64, device=dev),
                            "tg": torch.empty(ng, dtype=torch.float64, device=dev),
                            "host": torch.empty(ops.GA_ODE_CTL_WORDS, dtype=torch.float64).pin_memory()})
        y, out, k, ystage, tvec, ctl, tg, host = (rec.bufs[q] for q in ("y", "out", "k", "ystage", "tvec", "ctl", "tg", "host"))
        y.copy_(y0.detach().float())
        out[0].copy_(y)
        tg.copy_(torch.tensor(tt, dtype=torch.float64))
        nfe = [0]

        def velocity_into(dst, x, tv):
            nfe[0] += 1
            m.forward(x, tv, context, _step=_velocity_step(cfg_scale, cfg, dst))

        def rhs(ts, yy):      # (the two host-side evaluations of the initial step size)
            r = torch.empty_like(y)
            velocity_into(r, yy.contiguous(), torch.full((B,), float(ts), dtype=torch.float32, device=dev))
            return r

        tvec.fill_(tt[0])
        velocity_into(k[0], y, tvec)
        dt0 = _initial_step(rhs, tt[0], y, k[0], rtol, atol)
        head = torch.zeros(ops.GA_ODE_CTL_WORDS, dtype=torch.float64)
        head[ops.GA_ODE_T], head[ops.GA_ODE_DT], head[ops.GA_ODE_ATOL], head[ops.GA_ODE_RTOL], head[ops.GA_ODE_JNEXT] = tt[0], dt0, atol, rtol, 1
        ctl[:ops.GA_ODE_CTL_WORDS].copy_(head)
        evals_before = nfe[0]
        if ng > 1:
            if rec.graph is None:
                ode = ops.GaOdeDopri5(n, B, ng, y.data_ptr(), (ops.c_p * 7)(*[t.data_ptr() for t in k]), ystage.data_ptr(), tvec.data_ptr(),
                                      ctl.data_ptr(), tg.data_ptr(), out.data_ptr(), ctl.numel())

                def attempt():
                    stream = _stream(dev)
                    for i in range(6):
                        ops.check(Lib.ga_ode_dopri5_stage(ctypes.byref(ode), i, stream), "ga_ode_dopri5_stage")
                        velocity_into(k[i + 1], ystage, tvec)
                    ops.check(Lib.ga_ode_dopri5_finish(ctypes.byref(ode), stream), "ga_ode_dopri5_finish")

                # (capture executes nothing; the evaluations above were the warm-up, so it happens on the current stream)
                self._hold("dopri5", rec, capture_step(attempt, None, dev, warm_up=False), (ode,), context, *sig_args)
                nfe[0] = evals_before
            done_evt = torch.cuda.Event()
            while True:
                rec.graph.replay()
                host.copy_(ctl[:ops.GA_ODE_CTL_WORDS], non_blocking=True)
                done_evt.record()
                done_evt.synchronize()
                if host[ops.GA_ODE_DONE] != 0 or host[ops.GA_ODE_STEPS] >= max_steps:
                    break
            err, steps = int(host[ops.GA_ODE_ERROR]), int(host[ops.GA_ODE_STEPS])
            if err == 1:
                raise FloatingPointError(f"dopri5: non-finite error ratio at t = {float(host[ops.GA_ODE_T])}: the model returned NaN/inf")
            if err == 2:
                raise FloatingPointError(f"dopri5: step size underflow at t = {float(host[ops.GA_ODE_T])}")
            if host[ops.GA_ODE_DONE] == 0:
                raise RuntimeError(f"dopri5: more than {max_steps} attempted steps")
            if stats is not None:
                stats.update(nfe=evals_before + 6 * steps, steps=steps, rejected=int(host[ops.GA_ODE_REJECTED]), graph=True, device_loop=True,
                             ctl=[float(v) for v in host])     # the controller's scalar block after the last step (tests: bit-reproducible)
        elif stats is not None:
            stats.update(nfe=evals_before, steps=0, rejected=0, graph=True, device_loop=True)
        return out.clone()

    @torch.no_grad()
    def sde(self, x0, coef, context, method, last_step, cfg_scale, cfg, seed, noise, noise_out):
        """The reference's SDE sampling loop (``Sampler.sample_sde``, transport/transport.py:322-382: the stepper of
        transport/integrators.py:8-75 and one last step) with every step on the device (csrc/ode_sde.hip, GaSdeStep in
        include/ga_dit.h): a step is the function evaluation with the guided velocity leaving through the final-layer kernel, the
        Euler-Maruyama update (``method="Euler"``) or Heun's three phases around two evaluations (``"Heun"``) with the noise drawn
        inside the kernel, and the one-thread advance -- captured into ONE HIP graph and replayed for every interval, then the last
        step eagerly.  The step index, the coefficient table ``coef`` ([intervals + 1, GA_SDE_COEF_STRIDE] fp32, built by
        ``transport.sampler.sde_coefficients``), the seed and the initial state are device data rewritten per call: the captured step
        serves any seed, diffusion form and norm, and every replay draws fresh noise.  ``cfg``: the state is a doubled CFG batch whose
        halves take the same noise.  ``noise`` [intervals, n_draw]: normals to use instead; ``noise_out`` [intervals, n_draw]: receives
        the normals every step used.  Returns [intervals + 1, *x0.shape] fp32: slot k is the state after step k, the last slot the
        last step's output.  Bit-identical to the eager loop of ``transport/sampler.py`` on the same normals."""
        self._need_velocity("device-resident SDE sampler")
        m, dev = self.model, x0.device
        methods = ("Euler", "Heun")
        lasts = {"Mean": ops.GA_SDE_LAST_MEAN, "Tweedie": ops.GA_SDE_LAST_TWEEDIE, "Euler": ops.GA_SDE_LAST_EULER, None: ops.GA_SDE_LAST_NONE}
        if method not in methods or last_step not in lasts:
            raise ValueError(f"SDE sampler: method {method!r} / last step {last_step!r} (have {methods} / {tuple(lasts)})")
        ni = coef.shape[0] - 1
        if coef.dim() != 2 or coef.shape[1] != ops.GA_SDE_COEF_STRIDE or ni < 1:
            raise ValueError("coef is the [intervals + 1, GA_SDE_COEF_STRIDE] table of sde_coefficients")
        B, n = x0.shape[0], x0.numel()
        nd = n // 2 if cfg else n
        if cfg and B % 2:
            raise ValueError("a CFG state holds the conditional and the unconditional half")
        for name, t in (("noise", noise), ("noise_out", noise_out)):
            if t is not None and (t.numel() != ni * nd or t.shape[0] != ni):
                raise ValueError(f"{name} is [intervals = {ni}, n_draw = {nd}]")
        Lib = ops.lib()
        sig_args = (tuple(x0.shape), ni + 1, cfg, cfg_scale, (method, ni + 1, noise is not None, noise_out is not None))
        context, rec = self._begin("sde", context, *sig_args)
        if rec is None:
            y = torch.empty(tuple(x0.shape), dtype=torch.float32, device=dev)
            rec = HeldStep({"y": y, "vel": torch.empty_like(y), "k1": torch.empty_like(y), "xhat": torch.empty_like(y),
                            "out": torch.empty((ni + 1,) + tuple(y.shape), dtype=torch.float32, device=dev),
                            "counter": torch.zeros(1, dtype=torch.int32, device=dev), "tvec": torch.empty(B, dtype=torch.float32, device=dev),
                            "coef": torch.empty((ni + 1, ops.GA_SDE_COEF_STRIDE), dtype=torch.float32, device=dev),
                            "seed": torch.zeros(1, dtype=torch.int64, device=dev),
                            "noise": torch.empty((ni, nd), dtype=torch.float32, device=dev) if noise is not None else None,
                            "nout": torch.empty(nd, dtype=torch.float32, device=dev) if noise_out is not None else None})
        st = rec.bufs
        y, vel, out, counter, tvec, cf = (st[q] for q in ("y", "vel", "out", "counter", "tvec", "coef"))
        cf.copy_(coef.detach().to(torch.float32))
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        st["seed"].copy_(torch.tensor([seed - (1 << 64) if seed >> 63 else seed], dtype=torch.int64))
        if noise is not None:
            st["noise"].copy_(noise.detach().reshape(ni, nd))
        sde = ops.GaSdeStep(n, B, ni, 1 if cfg else 0, y.data_ptr(), vel.data_ptr(), st["k1"].data_ptr(), st["xhat"].data_ptr(),
                            out.data_ptr(), counter.data_ptr(), tvec.data_ptr(), cf.data_ptr(), st["seed"].data_ptr(),
                            st["noise"].data_ptr() if noise is not None else None, st["nout"].data_ptr() if noise_out is not None else None)
        vstep = _velocity_step(cfg_scale, cfg, vel)

        def phase(p):
            ops.check(Lib.ga_sde_step(ctypes.byref(sde), p, _stream(dev)), "ga_sde_step")

        def one_step():     # a single chain of launches
            if method == "Euler":
                m.forward(y, tvec, context, _step=vstep)
                phase(ops.GA_SDE_EM)
            else:
                phase(ops.GA_SDE_HEUN_PERTURB)
                m.forward(st["xhat"], tvec, context, _step=vstep)
                phase(ops.GA_SDE_HEUN_PREDICT)
                m.forward(y, tvec, context, _step=vstep)
                phase(ops.GA_SDE_HEUN_CORRECT)
            phase(ops.GA_SDE_ADVANCE)

        def reset():
            y.copy_(x0.detach().float())
            counter.zero_()
            tvec.copy_(cf[0, ops.GA_SDE_C_T].expand(B))

        if rec.graph is None:
            self._hold("sde", rec, capture_step(one_step, reset, dev), (), context, *sig_args)
        else:
            reset()
        for k in range(ni):
            rec.graph.replay()
            if noise_out is not None:
                noise_out[k].reshape(-1).copy_(st["nout"])
        if last_step is not None:
            m.forward(y, tvec, context, _step=vstep)      # (ADVANCE left t1 in tvec)
        phase(lasts[last_step])
        return out.clone()

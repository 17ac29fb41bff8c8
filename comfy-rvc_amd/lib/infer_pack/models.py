"""SynthesizerTrnMs{256,768}NSFsid on the HIP kernel graph.

Drop-in for the inference surface of reference lib/infer_pack/models.py:580-809: same constructor signature (the
`cpt["config"]` list splatted, `is_half` kwarg), `load_state_dict`, `eval/float/half/to`, and
`infer(phone, phone_lengths, pitch, nsff0, sid, rate=None)` returning `(o, x_mask, (z, z_p, m_p, logs_p))`.
The reference draws its noise from the global torch RNG inside `infer` (models.py:801 and :409); here the same two
draws are made on the host with the same shapes and order - or supplied explicitly through `noise=(noise_z, noise_src)`
(precedent: the reference's ONNX twin takes `rnd`, models_onnx.py:634-648).

The training forward (reference :665-680,:781-796, `_nono` :894-903,:1000-1009) is there too, without a backward pass:
`forward(phone, phone_lengths, pitch, pitchf, y, y_lengths, ds)` / `net_g(...)` returns
`(o, ids_slice, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q))` when the loaded state dict held `enc_q.*`.  The library is batch-1: the items of
a batch run one after the other on the current stream, each at its own length, into zero-filled padded outputs (what the reference's masks leave).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from ... import _lib


class _SynthesizerNSFsid:
    FEAT_DIM = 768
    HAS_F0 = True

    def __init__(self, spec_channels, segment_size, inter_channels, hidden_channels, filter_channels, n_heads, n_layers,
                 kernel_size, p_dropout, resblock, resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates,
                 upsample_initial_channel, upsample_kernel_sizes, spk_embed_dim, gin_channels, sr, device="cuda:0", trainable=False, **kwargs):
        if isinstance(sr, str):
            sr = {"32k": 32000, "40k": 40000, "48k": 48000}[sr]
        assert str(resblock) == "1", "only ResBlock1 generators are on the RVC inference path"
        assert len(resblock_kernel_sizes) == 3 and all(len(d) == 3 for d in resblock_dilation_sizes)
        assert len(upsample_rates) <= 8
        self.inter_channels, self.hidden_channels, self.sr = inter_channels, hidden_channels, sr
        self.spec_channels, self.segment_size, self.p_dropout = int(spec_channels), int(segment_size), float(p_dropout)
        self.upsample_rates = list(upsample_rates)
        self.gin_channels = int(gin_channels)
        self.upp = int(np.prod(upsample_rates))
        self.device = torch.device(device)
        cfg = _lib.SynthConfig()
        cfg.inter_channels, cfg.hidden_channels, cfg.filter_channels = inter_channels, hidden_channels, filter_channels
        cfg.n_heads, cfg.n_layers, cfg.kernel_size = n_heads, n_layers, kernel_size
        cfg.n_resblock_kernels = 3
        for i in range(3):
            cfg.resblock_kernel_sizes[i] = resblock_kernel_sizes[i]
            for j in range(3):
                cfg.resblock_dilations[i][j] = resblock_dilation_sizes[i][j]
        cfg.n_upsamples = len(upsample_rates)
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
        cfg.upsample_initial_channel, cfg.spk_embed_dim, cfg.gin_channels, cfg.sr = upsample_initial_channel, spk_embed_dim, gin_channels, sr
        cfg.feat_dim = self.FEAT_DIM
        cfg.spec_channels, cfg.segment_size = self.spec_channels, self.segment_size
        self._ctx = _lib.get_ctx(self.device.index or 0)
        h = C.c_void_p()
        _lib.check(_lib.lib.rvc_synth_create(self._ctx, C.byref(cfg), C.byref(h)))
        self._h = h
        self.trainable = bool(trainable)
        if self.trainable:                     # weight_v / weight_g of the decoder stay on the device, tapes record `sine` and `g`: what dec_weight_grad needs
            _lib.check(_lib.lib.rvc_synth_keep_parameters(self._h, 1))
        self._loaded = False
        self.enc_q = None   # `del net_g.enc_q` in get_vc (reference vc_infer_pipeline.py:219) must keep working

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None and getattr(_lib, 'lib', None) is not None:   # (module may be torn down at exit)
            _lib.lib.rvc_synth_destroy(h)
            self._h = None

    def load_state_dict(self, state_dict, strict=False):
        # the posterior encoder is loaded when the checkpoint has it and the caller has not deleted it (`del net_g.enc_q`, get_vc)
        keep_q = hasattr(self, "enc_q")
        sd = {k: v for k, v in state_dict.items() if keep_q or not k.startswith("enc_q.")}
        with torch.cuda.device(self.device):
            _lib.set_tensors(_lib.lib.rvc_synth_set_tensor, self._h, sd)
            _lib.check(_lib.lib.rvc_synth_finalize(self._h))
        has_f0 = bool(_lib.lib.rvc_synth_has_f0(self._h))
        if has_f0 != self.HAS_F0:      # the reference would fail in load_state_dict(strict) / at the first infer call
            raise ValueError(f"{type(self).__name__} expects a checkpoint trained {'with' if self.HAS_F0 else 'without'} f0 "
                             f"(cpt['f0'] = {int(self.HAS_F0)}), this one is the other family")
        self._loaded = True
        return self

    def eval(self):
        return self

    def float(self):
        return self

    def half(self):
        return self   # weights stay fp32 on the device: the fp32-MFMA graph is the parity path

    def to(self, device):
        return self

    def infer(self, phone, phone_lengths, pitch, nsff0, sid, rate=None, noise=None, taps=None, phone_channel_major=False, keep=None):
        """keep=(k0, k1): frames whose samples the caller keeps - only out[..., k0 * upp : k1 * upp] is defined then (rvc_synth_infer_window)."""
        assert self._loaded, "load_state_dict first"
        assert rate is None, "`rate` is unused by every caller of the reference (SURVEY 8a9)"
        dev = self.device
        if phone_channel_major:
            T = int(phone.shape[-1])
            ph = phone.to(dev, torch.float32).contiguous()
        else:
            assert phone.dim() == 3 and phone.shape[0] == 1
            T = int(phone.shape[1])
            ph = phone.to(dev, torch.float32).contiguous()
        assert int(phone_lengths.reshape(-1)[0]) == T, "only full-length sequences (the reference always passes p_len = T)"
        if noise is None:   # same draw order and shapes as the reference on its CPU path
            noise_z = torch.randn(1, self.inter_channels, T)
            torch.rand(1, 1)                                   # SineGen rand_ini (zeroed for harmonic_num = 0, models.py:378-381)
            noise_src = torch.randn(1, T * self.upp, 1)
        else:
            noise_z, noise_src = noise
        nz = torch.as_tensor(noise_z).to(dev, torch.float32).contiguous().view(self.inter_channels, T)
        ns = torch.as_tensor(noise_src).to(dev, torch.float32).contiguous().view(T * self.upp)
        pc = pitch.to(dev, torch.int64).contiguous().view(-1)[:T]
        pf = nsff0.to(dev, torch.float32).contiguous().view(-1)[:T]
        assert pc.numel() == T and pf.numel() == T
        out = torch.empty(1, 1, T * self.upp, dtype=torch.float32, device=dev)
        tp, tbuf = None, {}
        if taps is not None:
            C_, N = self.inter_channels, T * self.upp
            sizes = {"enc_p_layer0": (self.hidden_channels, T), "m_p": (C_, T), "logs_p": (C_, T), "z_p": (C_, T), "z": (C_, T),
                     "sine_waves": (N,), "har_source": (N,)}
            for n in taps:
                if n in sizes:
                    tbuf[n] = torch.empty(sizes[n], dtype=torch.float32, device=dev)
                else:
                    tbuf[n] = taps[n]
            tp = _lib.SynthTaps(*[_lib.ptr(tbuf.get(n)) for n, _ in _lib.SynthTaps._fields_])
        sid_i = int(torch.as_tensor(sid).reshape(-1)[0])
        with torch.cuda.device(dev):
            k0, k1 = (0, T) if keep is None else (int(keep[0]), int(keep[1]))
            _lib.check(_lib.lib.rvc_synth_infer_window(self._h, _lib.current_stream(), _lib.ptr(ph), 1 if phone_channel_major else 0,
                                                       _lib.ptr(pc), _lib.ptr(pf), sid_i, _lib.ptr(nz), _lib.ptr(ns), T, _lib.ptr(out),
                                                       C.byref(tp) if tp is not None else None, k0, k1))
        if taps is not None:
            taps.update(tbuf)
        x_mask = torch.ones(1, 1, T, dtype=torch.float32, device=dev)
        return out, x_mask, (tbuf.get("z"), tbuf.get("z_p"), tbuf.get("m_p"), tbuf.get("logs_p"))

    # ------------------------------------------------------------------------------------------- training forward
    def _forward(self, phone, phone_lengths, pitch, pitchf, y, y_lengths, ds, noise, ids_slice, with_tape=False, record_flow=False):
        """SynthesizerTrnMs{256,768}NSFsid[_nono].forward (reference :781-796,:894-903).  noise=(noise_q [B,inter,T], noise_src [B,seg*upp,1]);
        without it the draws are made on the host in the reference's order and shapes: enc_q's randn_like [B,inter,T] (:237), torch.rand([B]) of
        rand_slice_segments (commons.py:173), SineGen's rand_ini torch.rand(B, 1) (:378-381, zeroed) and its randn_like [B,seg*upp,1] (:409)."""
        assert self._loaded, "load_state_dict first"
        if self.p_dropout != 0:
            raise ValueError("the forward implements the dropout-free arithmetic: p_dropout must be 0 (it is in every shipped configuration)")
        if not _lib.lib.rvc_synth_has_posterior(self._h):
            raise RuntimeError("no posterior encoder: the loaded state dict had no enc_q.* tensors, or enc_q was deleted before loading")
        dev, seg, IC, upp = self.device, self.segment_size, self.inter_channels, self.upp
        pl = torch.as_tensor(phone_lengths).reshape(-1).to("cpu", torch.int64)
        yl = torch.as_tensor(y_lengths).reshape(-1).to("cpu", torch.int64)
        B = int(yl.numel())
        if pl.numel() != B or not torch.equal(pl, yl):
            raise ValueError("phone_lengths and y_lengths differ: the flow maps the posterior's frames onto the prior's one to one")
        if int(yl.min()) < seg:
            raise ValueError(f"an item is shorter than segment_size ({seg} frames)")
        Tx, Ty = int(phone.shape[1]), int(y.shape[2])
        assert phone.shape[0] == B and y.shape[0] == B and y.shape[1] == self.spec_channels and int(yl.max()) <= min(Tx, Ty)
        f0 = self.HAS_F0
        noise_q = noise_src = None
        if noise is not None:
            noise_q, noise_src = noise if isinstance(noise, (tuple, list)) else (noise, None)
        if noise_q is None:
            noise_q = torch.randn(B, IC, Ty)
        if ids_slice is None:
            ids_slice = (torch.rand([B]) * (yl - seg + 1)).to(dtype=torch.long)
        elif noise is None:
            torch.rand([B])
        if f0 and noise_src is None:
            torch.rand(B, 1)
            noise_src = torch.randn(B, seg * upp, 1)
        ids = torch.as_tensor(ids_slice).reshape(-1).to("cpu", torch.int64)
        assert ids.numel() == B
        ph = phone.to(dev, torch.float32)
        yd = y.to(dev, torch.float32)
        nq = torch.as_tensor(noise_q).to(dev, torch.float32)
        sid = torch.as_tensor(ds).reshape(-1).to("cpu", torch.int64)
        if f0:
            pc, pf = pitch.to(dev, torch.int64), pitchf.to(dev, torch.float32)
            ns = torch.as_tensor(noise_src).to(dev, torch.float32).reshape(B, seg * upp)
        o = torch.zeros(B, 1, seg * upp, dtype=torch.float32, device=dev)
        taps = [torch.zeros(B, IC, Ty, dtype=torch.float32, device=dev) for _ in range(6)]       # z, z_p, m_p, logs_p, m_q, logs_q
        tape = None
        if isinstance(with_tape, GeneratorTape):      # record again into the caller's tape: nothing is allocated
            tape = with_tape
            if tape.net is not self or tape.B != B:
                raise ValueError("the tape belongs to another net or another batch size")
            tape.ids, tape.Ty = [int(i) for i in ids], Ty
        elif with_tape:
            tape = GeneratorTape(self, B, ids, Ty)
        if tape is not None:
            tape.lengths, tape.flow_recorded = [int(v) for v in yl], False
        with torch.cuda.device(dev):
            st = _lib.current_stream()
            for b in range(B):
                L = int(yl[b])
                item = [torch.empty(IC, L, dtype=torch.float32, device=dev) for _ in range(6)]
                tp = _lib.SynthForwardTaps(*[_lib.ptr(t) for t in item])
                ph_b, y_b, nq_b = ph[b, :L].contiguous(), yd[b, :, :L].contiguous(), nq[b, :, :L].contiguous()
                pc_b = pc[b, :L].contiguous() if f0 else None
                pf_b = pf[b, :L].contiguous() if f0 else None
                ns_b = ns[b].contiguous() if f0 else None
                o_b = torch.empty(seg * upp, dtype=torch.float32, device=dev)
                if tape is not None and record_flow:      # and the flow's four couplings recorded for flow_input_grad
                    _lib.check(_lib.lib.rvc_synth_forward_tape_flow(self._h, st, _lib.ptr(ph_b), 0, _lib.ptr(pc_b), _lib.ptr(pf_b), _lib.ptr(y_b), int(sid[b]),
                                                                    _lib.ptr(nq_b), _lib.ptr(ns_b), L, int(ids[b]), _lib.ptr(o_b), C.byref(tp), tape._h[b], 1))
                elif tape is not None:      # the decoder layer by layer, recorded: y_hat is the taped wave
                    _lib.check(_lib.lib.rvc_synth_forward_tape(self._h, st, _lib.ptr(ph_b), 0, _lib.ptr(pc_b), _lib.ptr(pf_b), _lib.ptr(y_b), int(sid[b]),
                                                               _lib.ptr(nq_b), _lib.ptr(ns_b), L, int(ids[b]), _lib.ptr(o_b), C.byref(tp), tape._h[b]))
                else:
                    _lib.check(_lib.lib.rvc_synth_forward(self._h, st, _lib.ptr(ph_b), 0, _lib.ptr(pc_b), _lib.ptr(pf_b), _lib.ptr(y_b), int(sid[b]),
                                                          _lib.ptr(nq_b), _lib.ptr(ns_b), L, int(ids[b]), _lib.ptr(o_b), C.byref(tp)))
                o[b, 0] = o_b
                for dst, src in zip(taps, item):
                    dst[b, :, :L] = src
        x_mask = (torch.arange(Tx)[None, :] < pl[:, None]).to(torch.float32).unsqueeze(1).to(dev)
        y_mask = (torch.arange(Ty)[None, :] < yl[:, None]).to(torch.float32).unsqueeze(1).to(dev)
        res = (o, ids.to(dev), x_mask, y_mask, tuple(taps))
        if tape is not None:
            tape.flow_recorded = bool(record_flow)
        return (res, tape) if with_tape else res

    def forward(self, phone, phone_lengths, pitch, pitchf, y, y_lengths, ds, noise=None, ids_slice=None):
        return self._forward(phone, phone_lengths, pitch, pitchf, y, y_lengths, ds, noise, ids_slice)

    # ------------------------------------------------------------------------------------------- the decoder's backward data pass
    def forward_with_tape(self, phone, phone_lengths, pitch, pitchf, y, y_lengths, ds, noise=None, ids_slice=None, tape=None, record_flow=False):
        """forward's arguments -> (forward's 5-tuple, GeneratorTape).  The decoder runs layer by layer and records what its backward reads
        (rvc_synth_forward_tape); `o` is the taped wave, inside the 1e-3 gate of forward's but not bit-equal to it (forward keeps its fused ResBlock kernels).
        tape: a GeneratorTape of an earlier call with the same batch size to record into again (a trainer keeps one), instead of a new one.
        record_flow: the tape also records, per item at its own length, what flow_input_grad reads (rvc_synth_forward_tape_flow); z_p is then inside the 1e-3
        gate of a non-recording call's (the recording pass gates the WaveNet layers in a launch of its own), z and `o` keep their bits."""
        return self._forward(phone, phone_lengths, pitch, pitchf, y, y_lengths, ds, noise, ids_slice, with_tape=tape if tape is not None else True,
                             record_flow=record_flow)

    def dec_input_grad(self, tape, d_y_hat, return_deltas=False):
        """d_y_hat [B,1,seg*upp] -> (dz [B,inter,Ty], dg [B,gin], dhar [B,seg*upp] or None for a no-f0 net): the decoder's vector-Jacobian product
        (rvc_synth_dec_input_grad).  dz holds the slice's gradient at frames [ids, ids + seg) and zero elsewhere: what autograd leaves in z.grad from the decoder
        branch.  dg flows into emb_g's row; dhar stops at the harmonic source.  return_deltas: also a list of B dicts name -> copy of the tape's delta."""
        if not isinstance(tape, GeneratorTape) or tape.net is not self:
            raise ValueError("dec_input_grad: the tape belongs to another net")
        dev, seg, IC, upp, B = self.device, self.segment_size, self.inter_channels, self.upp, tape.B
        d = torch.as_tensor(d_y_hat).to(dev, torch.float32).reshape(B, seg * upp).contiguous()
        dz = torch.zeros(B, IC, tape.Ty, dtype=torch.float32, device=dev)
        dg = torch.empty(B, self.gin_channels, dtype=torch.float32, device=dev)
        dhar = torch.empty(B, seg * upp, dtype=torch.float32, device=dev) if self.HAS_F0 else None
        with torch.cuda.device(dev):
            st = _lib.current_stream()
            for b in range(B):
                dz_b = torch.empty(IC, seg, dtype=torch.float32, device=dev)
                _lib.check(_lib.lib.rvc_synth_dec_input_grad(self._h, st, tape._h[b], _lib.ptr(d[b]), _lib.ptr(dz_b), None, _lib.ptr(dg[b]),
                                                             _lib.ptr(dhar[b]) if dhar is not None else None))
                i0 = int(tape.ids[b])
                dz[b, :, i0:i0 + seg] = dz_b
        if return_deltas:
            return dz, dg, dhar, [{n: tape.tensor(b, n) for n in tape.delta_names()} for b in range(B)]
        return dz, dg, dhar

    # ------------------------------------------------------------------------------------------- the flow's backward data pass
    def flow_input_grad(self, tape, d_z_p, return_deltas=False):
        """d_z_p [B,inter,Ty] -> (dz_flow [B,inter,Ty], dg_flow [B,gin]): the vector-Jacobian product of the flow (rvc_synth_flow_input_grad) on a tape recorded
        with record_flow=True.  Each item runs at its own length; everything behind it is exactly 0 in dz_flow.  dz_flow is added to dec_input_grad's dz, dg_flow
        to its dg.  return_deltas: also a list of B dicts name -> copy of the tape's flow delta (GeneratorTape.flow_delta_names())."""
        if not isinstance(tape, GeneratorTape) or tape.net is not self:
            raise ValueError("flow_input_grad: the tape belongs to another net")
        if not getattr(tape, "flow_recorded", False):
            raise ValueError("flow_input_grad: the tape was recorded without record_flow=True")
        dev, IC, B = self.device, self.inter_channels, tape.B
        d = torch.as_tensor(d_z_p)
        if tuple(d.shape) != (B, IC, tape.Ty):
            raise ValueError(f"flow_input_grad: d_z_p must have the shape {(B, IC, tape.Ty)}, got {tuple(d.shape)}")
        d = d.to(dev, torch.float32)
        dz = torch.zeros(B, IC, tape.Ty, dtype=torch.float32, device=dev)
        dg = torch.empty(B, self.gin_channels, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.current_stream()
            for b in range(B):
                L = tape.lengths[b]
                d_b = d[b, :, :L].contiguous()
                dz_b = torch.empty(IC, L, dtype=torch.float32, device=dev)
                _lib.check(_lib.lib.rvc_synth_flow_input_grad(self._h, st, tape._h[b], _lib.ptr(d_b), L, _lib.ptr(dz_b), _lib.ptr(dg[b])))
                dz[b, :, :L] = dz_b
        if return_deltas:
            return dz, dg, [{n: tape.tensor(b, n) for n in tape.flow_delta_names()} for b in range(B)]
        return dz, dg

    def flow_backward_launch_count(self):
        """Kernel launches of one item's flow_input_grad (rvc_synth_flow_input_grad_launch_count): a constant of the net, whatever the batch and the lengths."""
        n = int(_lib.lib.rvc_synth_flow_input_grad_launch_count(self._h))
        if n < 0:
            _lib.check(1)
        return n

    def dec_backward_launch_count(self):
        n = int(_lib.lib.rvc_synth_dec_input_grad_launch_count(self._h))
        if n < 0:
            _lib.check(1)
        return n

    # ------------------------------------------------------------------------------------------- the decoder's weight-gradient pass
    MAX_WGRAD_ITEMS = 16

    def dec_parameter_shapes(self):
        """OrderedDict name -> shape of the dec.* parameter tensors in the reference module's state-dict order (rvc_synth_dec_param_info)."""
        assert self._loaded, "load_state_dict first"
        out = OrderedDict()
        name, shape, ndim = C.create_string_buffer(128), (_lib.c_int64 * 8)(), C.c_int()
        n = _lib.lib.rvc_synth_dec_param_count(self._h)
        if n < 0:
            _lib.check(1)
        for k in range(n):
            _lib.check(_lib.lib.rvc_synth_dec_param_info(self._h, k, name, 128, shape, C.byref(ndim)))
            out[name.value.decode()] = tuple(int(shape[i]) for i in range(ndim.value))
        return out

    def dec_weight_grad(self, tape):
        """The gradient with respect to every dec.* parameter, summed over the tape's items (rvc_synth_dec_weight_grad): an OrderedDict from state-dict name to a
        float32 device tensor in the parameter's shape, views of ONE contiguous buffer in dec_parameter_shapes() order (`.flat` of the result holds it).  The tape
        must have been through dec_input_grad since its last forward_with_tape: the deltas it reads are that pass's.  Needs trainable=True."""
        assert self._loaded, "load_state_dict first"
        if not self.trainable:
            raise ValueError("dec_weight_grad: the net was built without trainable=True (weight_v / weight_g are not kept on the device)")
        if not isinstance(tape, GeneratorTape) or tape.net is not self:
            raise ValueError("dec_weight_grad: the tape belongs to another net")
        return self._dec_weight_grad(tape._h)

    def _dec_weight_grad(self, handles):
        dev = self.device
        params = self.dec_parameter_shapes()
        sizes = [int(np.prod(s)) for s in params.values()]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        out, o = _GradDict(), 0
        for (name, shape), n in zip(params.items(), sizes):
            out[name] = flat[o:o + n].view(shape)
            o += n
        out.flat = flat
        pt = (C.c_void_p * max(1, len(handles)))(*[h.value if isinstance(h, C.c_void_p) else h for h in handles])
        pg = (C.c_void_p * len(out))(*[t.data_ptr() for t in out.values()])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.rvc_synth_dec_weight_grad(self._h, _lib.current_stream(), pt, len(handles), pg))
        return out

    def dec_weight_grad_launch_count(self):
        """Kernel launches of one dec_weight_grad (rvc_synth_dec_weight_grad_launch_count): a constant of the net, whatever the batch and the segment."""
        n = int(_lib.lib.rvc_synth_dec_weight_grad_launch_count(self._h))
        if n < 0:
            _lib.check(1)
        return n

    # ------------------------------------------------------------------------------------------- the flow's weight-gradient pass
    def flow_parameter_shapes(self):
        """OrderedDict name -> shape of the 100 flow.* parameter tensors in the reference module's state-dict order (rvc_synth_flow_param_info)."""
        assert self._loaded, "load_state_dict first"
        out = OrderedDict()
        name, shape, ndim = C.create_string_buffer(128), (_lib.c_int64 * 8)(), C.c_int()
        n = _lib.lib.rvc_synth_flow_param_count(self._h)
        if n < 0:
            _lib.check(1)
        for k in range(n):
            _lib.check(_lib.lib.rvc_synth_flow_param_info(self._h, k, name, 128, shape, C.byref(ndim)))
            out[name.value.decode()] = tuple(int(shape[i]) for i in range(ndim.value))
        return out

    def flow_weight_grad(self, tape):
        """The gradient with respect to every flow.* parameter, summed over the tape's items, each at its own length (rvc_synth_flow_weight_grad): an OrderedDict
        from state-dict name to a float32 device tensor in the parameter's shape, views of ONE contiguous buffer in flow_parameter_shapes() order (`.flat`).  The
        tape must have been recorded with record_flow=True and been through flow_input_grad since.  Needs trainable=True."""
        assert self._loaded, "load_state_dict first"
        if not self.trainable:
            raise ValueError("flow_weight_grad: the net was built without trainable=True (weight_v / weight_g are not kept on the device)")
        if not isinstance(tape, GeneratorTape) or tape.net is not self:
            raise ValueError("flow_weight_grad: the tape belongs to another net")
        if not getattr(tape, "flow_recorded", False):
            raise ValueError("flow_weight_grad: the tape was recorded without record_flow=True")
        return self._flow_weight_grad(tape._h)

    def _flow_weight_grad(self, handles):
        dev = self.device
        params = self.flow_parameter_shapes()
        sizes = [int(np.prod(s)) for s in params.values()]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        out, o = _GradDict(), 0
        for (name, shape), n in zip(params.items(), sizes):
            out[name] = flat[o:o + n].view(shape)
            o += n
        out.flat = flat
        pt = (C.c_void_p * max(1, len(handles)))(*[h.value if isinstance(h, C.c_void_p) else h for h in handles])
        pg = (C.c_void_p * len(out))(*[t.data_ptr() for t in out.values()])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.rvc_synth_flow_weight_grad(self._h, _lib.current_stream(), pt, len(handles), pg))
        return out

    def flow_weight_grad_launch_count(self):
        """Kernel launches of one flow_weight_grad (rvc_synth_flow_weight_grad_launch_count): a constant of the net, whatever the batch and the lengths."""
        n = int(_lib.lib.rvc_synth_flow_weight_grad_launch_count(self._h))
        if n < 0:
            _lib.check(1)
        return n

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


def flow_parameter_spec(config):
    """OrderedDict name -> shape of the flow's parameter tensors (ResidualCouplingBlock, reference lib/infer_pack/models.py:150-196; WN modules.py:130-182) for a
    constructor argument list, in the reference module's state-dict order: what flow_parameter_shapes() reports for a loaded net, computed on the host."""
    inter, hidden, gin = config[2], config[3], config[16]
    s, half = OrderedDict(), inter // 2

    def wn(p, shape):
        s[p + ".bias"], s[p + ".weight_g"], s[p + ".weight_v"] = (shape[0],), (shape[0], 1, 1), shape
    for f in range(4):
        p = f"flow.flows.{2 * f}."
        s[p + "pre.weight"], s[p + "pre.bias"] = (hidden, half, 1), (hidden,)
        for i in range(3):
            wn(p + f"enc.in_layers.{i}", (2 * hidden, hidden, 5))
        for i in range(3):
            wn(p + f"enc.res_skip_layers.{i}", (2 * hidden if i < 2 else hidden, hidden, 1))
        wn(p + "enc.cond_layer", (6 * hidden, gin, 1))
        s[p + "post.weight"], s[p + "post.bias"] = (half, hidden, 1), (half,)
    return s


def dec_parameter_spec(config, f0=True):
    """OrderedDict name -> shape of the decoder's parameter tensors (GeneratorNSF / Generator, reference lib/infer_pack/models.py:460-566,:244-311) for a
    constructor argument list, in the reference module's state-dict order: what dec_parameter_shapes() reports for a loaded net, computed on the host."""
    inter, rb_k, up_rates, up_init, up_k, gin = config[2], config[10], config[12], config[13], config[14], config[16]
    nu, s = len(up_rates), OrderedDict()
    if f0:
        s["dec.m_source.l_linear.weight"], s["dec.m_source.l_linear.bias"] = (1, 1), (1,)
        for i in range(nu):
            s[f"dec.noise_convs.{i}.weight"] = (up_init >> (i + 1), 1, 2 * int(np.prod(up_rates[i + 1:])) if i + 1 < nu else 1)
            s[f"dec.noise_convs.{i}.bias"] = (up_init >> (i + 1),)
    s["dec.conv_pre.weight"], s["dec.conv_pre.bias"] = (up_init, inter, 7), (up_init,)

    def wn(p, shape):
        s[p + ".bias"] = (shape[1],) if ".ups." in p else (shape[0],)
        s[p + ".weight_g"], s[p + ".weight_v"] = (shape[0], 1, 1), shape
    for i in range(nu):
        wn(f"dec.ups.{i}", (up_init >> i, up_init >> (i + 1), up_k[i]))
    for i in range(nu):
        for j, k in enumerate(rb_k):
            for cs in ("convs1", "convs2"):
                for m in range(3):
                    wn(f"dec.resblocks.{i * len(rb_k) + j}.{cs}.{m}", (up_init >> (i + 1), up_init >> (i + 1), k))
    s["dec.conv_post.weight"] = (1, up_init >> nu, 7)
    s["dec.cond.weight"], s["dec.cond.bias"] = (up_init, gin, 1), (up_init,)
    return s


class GeneratorTape:
    """The recorded decoder passes of one batch (forward_with_tape): B rvc_gen_tape handles, one per item, and the slice starts `ids`.  `tensor(b, name)` is a
    copy of item b's tensor - activations z, har, pre, up{i}, rb{i}.{j}.y{m}, rb{i}.{j}.t{m}, out{i}, y_hat and, after dec_input_grad, the deltas
    d.post, d.out{i}, d.rb{i}.{j}.t{m}, d.rb{i}.{j}.y{m}, d.up{i}, d.pre, d.cond, d.g, d.har (include/rvc_hip.h).  `nbytes`: device bytes of the B tapes."""

    def __init__(self, net, B, ids, Ty):
        self.net, self.B, self.ids, self.Ty = net, int(B), [int(i) for i in ids], int(Ty)
        self._h = []
        with torch.cuda.device(net.device):
            for _ in range(self.B):
                h = C.c_void_p()
                _lib.check(_lib.lib.rvc_gen_tape_create(net._h, C.byref(h)))
                self._h.append(h)

    def __del__(self):
        if _lib is not None and getattr(_lib, 'lib', None) is not None:
            for h in getattr(self, "_h", []):
                _lib.lib.rvc_gen_tape_release(h)
            self._h = []

    @property
    def nbytes(self):
        return sum(int(_lib.lib.rvc_gen_tape_bytes(h)) for h in self._h)

    def tensor(self, b, name):
        p, rows, cols = C.c_void_p(), C.c_int(), C.c_int64()
        _lib.check(_lib.lib.rvc_gen_tape_tensor(self._h[b], name.encode(), C.byref(p), C.byref(rows), C.byref(cols)))
        return _lib.device_view(p.value, (rows.value, cols.value), self.net.device)

    def set_timing(self, on=True):
        """HIP events around the taped decoder and at the backward's stage boundaries of every item (rvc_gen_tape_timing); off by default."""
        for h in self._h:
            _lib.check(_lib.lib.rvc_gen_tape_timing(h, 1 if on else 0))

    def times(self, b):
        """Milliseconds of item b's last passes (waits for them): {"decoder_forward": .., "backward": {"post": .., "stage3": .., .., "stage0": .., "pre": ..}};
        {} when nothing was recorded."""
        buf = (C.c_float * 16)()
        n = int(_lib.lib.rvc_gen_tape_times(self._h[b], buf, 16))
        if n < 0:
            _lib.check(1)
        if n == 0:
            return {}
        nu = len(self.net.upsample_rates)
        names = ["post"] + [f"stage{i}" for i in range(nu - 1, -1, -1)] + ["pre"]
        return {"decoder_forward": float(buf[0]), "backward": {k: float(buf[1 + i]) for i, k in enumerate(names[:n - 1])}}

    def wgrad_times(self):
        """Milliseconds of the last dec_weight_grad on this tape (timing on; waits for it): {"stage0": .., .., "rest": ..} - per stage the up-sampler and its
        ResBlocks, then conv_pre and the direct kernels; {} when nothing was recorded."""
        buf = (C.c_float * 16)()
        n = int(_lib.lib.rvc_gen_tape_wgrad_times(self._h[0], buf, 16))
        if n < 0:
            _lib.check(1)
        names = [f"stage{i}" for i in range(len(self.net.upsample_rates))] + ["rest"]
        return {k: float(buf[i]) for i, k in enumerate(names[:n])}

    def _names(self, deltas):
        net, out = self.net, []
        d = "d." if deltas else ""
        if not deltas:
            out += ["z"] + (["har"] if net.HAS_F0 else [])
        out.append(d + "pre")
        for i in range(len(net.upsample_rates)):
            out.append(f"{d}up{i}")
            for j in range(3):
                out += [f"{d}rb{i}.{j}.y{m}" for m in (1, 2)] + [f"{d}rb{i}.{j}.t{m}" for m in range(3)]
            out.append(f"{d}out{i}")
        out.append("d.post" if deltas else "y_hat")
        if deltas:
            out += ["d.cond", "d.g"] + (["d.har"] if net.HAS_F0 else [])
        return out

    def activation_names(self):
        return self._names(False)

    def delta_names(self):
        return self._names(True)

    def flow_activation_names(self):
        """what a forward with record_flow=True leaves per item: pre's output, each WaveNet layer's input (x0 is h0) and pre-gate activation, per coupling f"""
        return [f"flow{f}.{n}" for f in range(4) for n in ["h0"] + [f"x{i}" for i in range(3)] + [f"a{i}" for i in range(3)]]

    def flow_delta_names(self):
        """what flow_input_grad leaves per item: post's output cotangent, each layer's d a, pre's output cotangent, cond_layer's, and the item's dg"""
        return [f"d.flow{f}.{n}" for f in range(4) for n in ["m"] + [f"a{i}" for i in range(3)] + ["h0", "gc"]] + ["d.flow.g"]

    def flow_wgrad_names(self):
        """what a trainable net's tape additionally holds per item for flow_weight_grad: pre's and post's inputs from the recording forward, and from
        flow_input_grad the x-chain cotangent at the input of layers 1 and 2 and post^T d m (the skip half of every res_skip layer's output cotangent)"""
        return [f"flow{f}.{n}" for f in range(4) for n in ("xin", "out")] + [f"d.flow{f}.{n}" for f in range(4) for n in ("x1", "x2", "skip")]

    def flow_times(self, b):
        """Milliseconds of item b's recorded flow forward and last flow backward (set_timing on; waits for them): {"flow_forward": .., "flow_backward": ..}."""
        buf = (C.c_float * 2)()
        n = int(_lib.lib.rvc_gen_tape_flow_times(self._h[b], buf, 2))
        if n < 0:
            _lib.check(1)
        return {k: float(buf[i]) for i, k in enumerate(["flow_forward", "flow_backward"][:n])}


class _SynthesizerNSFsid_nono(_SynthesizerNSFsid):
    """No-f0 family (reference lib/infer_pack/models.py:812-1022): text encoder without pitch embedding, plain HiFi-GAN Generator.
    The reference's constructor has `sr=None` last (:833,:939); `infer(phone, phone_lengths, sid, rate=None)` draws one randn_like."""
    HAS_F0 = False

    def __init__(self, *config, sr=None, **kwargs):
        if len(config) == 18:
            config, sr = config[:17], config[17]
        super().__init__(*config, sr if sr is not None else 40000, **kwargs)

    def infer(self, phone, phone_lengths, sid, rate=None, noise=None, taps=None, phone_channel_major=False, keep=None):
        assert self._loaded, "load_state_dict first"
        assert rate is None, "`rate` is unused by every caller of the reference (SURVEY 8a9)"
        dev = self.device
        T = int(phone.shape[-1]) if phone_channel_major else int(phone.shape[1])
        ph = phone.to(dev, torch.float32).contiguous()
        assert int(torch.as_tensor(phone_lengths).reshape(-1)[0]) == T, "only full-length sequences (the reference always passes p_len = T)"
        noise_z = torch.randn(1, self.inter_channels, T) if noise is None else (noise[0] if isinstance(noise, (tuple, list)) else noise)
        nz = torch.as_tensor(noise_z).to(dev, torch.float32).contiguous().view(self.inter_channels, T)
        out = torch.empty(1, 1, T * self.upp, dtype=torch.float32, device=dev)
        tp, tbuf = None, {}
        if taps is not None:
            C_ = self.inter_channels
            sizes = {"enc_p_layer0": (self.hidden_channels, T), "m_p": (C_, T), "logs_p": (C_, T), "z_p": (C_, T), "z": (C_, T)}
            tbuf = {n: torch.empty(sizes[n], dtype=torch.float32, device=dev) for n in taps if n in sizes}
            tp = _lib.SynthTaps(*[_lib.ptr(tbuf.get(n)) for n, _ in _lib.SynthTaps._fields_])
        sid_i = int(torch.as_tensor(sid).reshape(-1)[0])
        with torch.cuda.device(dev):
            k0, k1 = (0, T) if keep is None else (int(keep[0]), int(keep[1]))
            _lib.check(_lib.lib.rvc_synth_infer_window(self._h, _lib.current_stream(), _lib.ptr(ph), 1 if phone_channel_major else 0, None, None, sid_i,
                                                       _lib.ptr(nz), None, T, _lib.ptr(out), C.byref(tp) if tp is not None else None, k0, k1))
        if taps is not None:
            taps.update(tbuf)
        x_mask = torch.ones(1, 1, T, dtype=torch.float32, device=dev)
        return out, x_mask, (tbuf.get("z"), tbuf.get("z_p"), tbuf.get("m_p"), tbuf.get("logs_p"))

    def forward(self, phone, phone_lengths, y, y_lengths, ds, *extra, noise=None, ids_slice=None):
        """Five arguments (reference :894,:1000): the no-f0 family has no pitch inputs; noise = noise_q alone (one randn_like, then the slice's rand)."""
        if extra:
            raise ValueError("no-f0 model: forward(phone, phone_lengths, y, y_lengths, ds) takes no pitch arguments")
        return self._forward(phone, phone_lengths, None, None, y, y_lengths, ds, noise, ids_slice)

    def forward_with_tape(self, phone, phone_lengths, y, y_lengths, ds, *extra, noise=None, ids_slice=None, tape=None, record_flow=False):
        if extra:
            raise ValueError("no-f0 model: forward_with_tape(phone, phone_lengths, y, y_lengths, ds) takes no pitch arguments")
        return self._forward(phone, phone_lengths, None, None, y, y_lengths, ds, noise, ids_slice, with_tape=tape if tape is not None else True,
                             record_flow=record_flow)


class SynthesizerTrnMs768NSFsid_nono(_SynthesizerNSFsid_nono):
    FEAT_DIM = 768


class SynthesizerTrnMs256NSFsid_nono(_SynthesizerNSFsid_nono):
    FEAT_DIM = 256


class SynthesizerTrnMs768NSFsid(_SynthesizerNSFsid):
    """v2: 768-d ContentVec features (reference lib/infer_pack/models.py:696-809)."""
    FEAT_DIM = 768


class SynthesizerTrnMs256NSFsid(_SynthesizerNSFsid):
    """v1: 256-d final_proj features (reference lib/infer_pack/models.py:580-693)."""
    FEAT_DIM = 256


# ------------------------------------------------------------------------------------------------- discriminators
class _MultiPeriodDiscriminator:
    """MultiPeriodDiscriminator / MultiPeriodDiscriminatorV2 (reference lib/infer_pack/models.py:1024-1145), forward and input gradient: DiscriminatorS plus one
    DiscriminatorP per period.  `forward(y, y_hat)` / `net_d(y, y_hat)` returns `(y_d_rs, y_d_gs, fmap_rs, fmap_gs)` like the reference: per
    sub-discriminator the score [B, H p] of the real and of the generated batch and the lists of feature maps ([B,C,H,p]; [B,C,T'] for
    DiscriminatorS).  `input_grad(fmaps, tap_cotangents)` is the one backward pass: the gradient with respect to the input waveform (rvc_disc_input_grad).  Both batches run through every layer in one launch (rvc_disc_forward on the 2 B signals); the returned tensors are views of
    the buffers the layers wrote.  `trainable=True` keeps weight_v / weight_g on the device (about the weights' size again) and allows
    `weight_grad(x, fmaps, deltas)`, the gradient with respect to every parameter (rvc_disc_weight_grad); without it a loaded net is what it was.  A trainable
    net can be stepped (lib.train.optim.AdamW over rvc_disc_adamw_step) and read back: `state_dict()`, `get_parameters()`, `load_parameters(flat)`.
    CUDA tensors only: there is no CPU path."""
    VERSION = 1

    def __init__(self, use_spectral_norm=False, device="cuda:0", trainable=False):
        if use_spectral_norm:
            raise NotImplementedError("spectral norm is not implemented (use_spectral_norm is false in every shipped configuration)")
        self.device = torch.device(device)
        self._ctx = _lib.get_ctx(self.device.index or 0)
        h = C.c_void_p()
        _lib.check(_lib.lib.rvc_disc_create(self._ctx, self.VERSION, C.byref(h)))
        self._h = h
        self.trainable = bool(trainable)
        if self.trainable:                     # weight_v / weight_g stay on the device (about the weights' size again): what weight_grad needs
            _lib.check(_lib.lib.rvc_disc_keep_parameters(self._h, 1))
        self._loaded = False
        self.periods = [2, 3, 5, 7, 11, 17] + ([23, 37] if self.VERSION == 2 else [])

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None and getattr(_lib, 'lib', None) is not None:
            _lib.lib.rvc_disc_release(h)
            self._h = None

    def load_state_dict(self, state_dict, strict=False):
        with torch.cuda.device(self.device):
            _lib.set_tensors(_lib.lib.rvc_disc_set_tensor, self._h, state_dict)
            _lib.check(_lib.lib.rvc_disc_finalize(self._h))
        self._loaded = True
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def to(self, device):
        return self

    def launch_count(self, S, T):
        """Kernel launches of one forward over S signals of T samples (rvc_disc_launch_count: the size of the plan; nothing is launched)."""
        n = _lib.lib.rvc_disc_launch_count(self._h, int(S), int(T))
        if n < 0:
            raise _lib.RvcHipError(_lib.lib.rvc_last_error().decode("utf-8", "replace"))
        return n

    def tap_shapes(self, T):
        """[[(C, H, p) per tap] per sub-discriminator] for signals of T samples."""
        out = []
        for i in range(_lib.lib.rvc_disc_count(self._h)):
            rows = []
            for l in range(_lib.lib.rvc_disc_num_taps(self._h, i)):
                c, h, p = C.c_int(), C.c_int(), C.c_int()
                _lib.check(_lib.lib.rvc_disc_tap_shape(self._h, i, l, int(T), C.byref(c), C.byref(h), C.byref(p)))
                rows.append((c.value, h.value, p.value))
            out.append(rows)
        return out

    def _run(self, sig):
        """sig [S, T] float32 contiguous on the device -> [[tap buffers [S,C,H,p] ([S,C,T'] for DiscriminatorS)] per sub-discriminator], one rvc_disc_forward"""
        S_, T, dev = int(sig.shape[0]), int(sig.shape[1]), sig.device
        shapes = self.tap_shapes(T)
        bufs = [[torch.empty((S_, c, h, p) if i else (S_, c, h), dtype=torch.float32, device=dev) for (c, h, p) in rows] for i, rows in enumerate(shapes)]
        flat = [t for rows in bufs for t in rows]
        ptrs = (C.c_void_p * len(flat))(*[t.data_ptr() for t in flat])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.rvc_disc_forward(self._h, _lib.current_stream(), _lib.ptr(sig), S_, T, None, ptrs))
        return bufs

    def forward_single(self, x):
        """One batch x [B,1,T] alone through every sub-discriminator (S = B signals): the lists of feature maps, the score being the last of each list.
        What input_grad needs when only one half matters (gradient_norm_loss)."""
        assert self._loaded, "load_state_dict first"
        if not (hasattr(x, "is_cuda") and x.is_cuda):
            raise ValueError("the discriminators run on the device: pass CUDA tensors (there is no CPU path)")
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"x must be [B, 1, T]: got {tuple(x.shape)}")
        B, T = int(x.shape[0]), int(x.shape[2])
        for p in self.periods:
            if (p - T % p) % p >= T:
                raise ValueError(f"T = {T} is not longer than the reflect pad period {p} needs")
        return self._run(x.detach().to(torch.float32).reshape(B, T).contiguous())

    def forward(self, y, y_hat):
        assert self._loaded, "load_state_dict first"
        for t in (y, y_hat):
            if not (hasattr(t, "is_cuda") and t.is_cuda):
                raise ValueError("the discriminators run on the device: pass CUDA tensors (there is no CPU path)")
        if y.dim() != 3 or y.shape[1] != 1 or tuple(y.shape) != tuple(y_hat.shape):
            raise ValueError(f"y and y_hat must both be [B, 1, T]: got {tuple(y.shape)} and {tuple(y_hat.shape)}")
        B, T = int(y.shape[0]), int(y.shape[2])
        for p in self.periods:
            if (p - T % p) % p >= T:
                raise ValueError(f"T = {T} is not longer than the reflect pad period {p} needs")
        sig = torch.cat([y.detach().to(torch.float32).reshape(B, T), y_hat.detach().to(torch.float32).reshape(B, T)]).contiguous()
        bufs = self._run(sig)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for rows in bufs:
            fmap_rs.append([t[:B] for t in rows])
            fmap_gs.append([t[B:] for t in rows])
            y_d_rs.append(torch.flatten(rows[-1][:B], 1, -1))
            y_d_gs.append(torch.flatten(rows[-1][B:], 1, -1))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    def backward_launch_count(self, S, T):
        """Kernel launches of one input_grad over S signals of T samples (rvc_disc_input_grad_launch_count: the size of the plan; nothing is launched)."""
        n = _lib.lib.rvc_disc_input_grad_launch_count(self._h, int(S), int(T))
        if n < 0:
            raise _lib.RvcHipError(_lib.lib.rvc_last_error().decode("utf-8", "replace"))
        return n

    def input_grad(self, fmaps, tap_cotangents, return_deltas=False):
        """The vector-Jacobian product of the forward with respect to its input (rvc_disc_input_grad).  fmaps: the lists of feature maps `forward` returned
        for ONE half (fmap_rs or fmap_gs: leading-dimension slices, hence contiguous); tap_cotangents: the same structure, each entry the cotangent of that
        feature map in its shape (the last of a sub-discriminator is dL/dscore, [B, H p] accepted) or None for zero.  Returns dL/dinput [B, 1, T] float32;
        return_deltas: also the per-layer dL/d(pre-activation) buffers the pass wrote, in the taps' structure.  The leaky ReLU masks are read from the
        feature maps, so the result is the exact gradient of what the forward computed."""
        assert self._loaded, "load_state_dict first"
        if len(fmaps) != len(self.periods) + 1 or len(tap_cotangents) != len(fmaps) or any(len(a) != len(b) for a, b in zip(fmaps, tap_cotangents)):
            raise ValueError("input_grad: fmaps and tap_cotangents must both hold one list per sub-discriminator with one entry per tap")
        first = fmaps[0][0] if len(fmaps[0]) else None
        if first is None or not (hasattr(first, "is_cuda") and first.is_cuda) or first.dim() != 3:
            raise ValueError("input_grad: device feature maps as forward returned them expected (there is no CPU path)")
        B, T, dev = int(first.shape[0]), int(first.shape[2]), first.device
        for p in self.periods:
            if (p - T % p) % p >= T:
                raise ValueError(f"T = {T} is not longer than the reflect pad period {p} needs")
        shapes = self.tap_shapes(T)
        if [len(r) for r in shapes] != [len(r) for r in fmaps]:
            raise ValueError("input_grad: wrong number of feature maps")
        flat_f, flat_c = [], []
        for i, rows in enumerate(shapes):
            for l, (c, h, p) in enumerate(rows):
                want = (B, c, h, p) if i else (B, c, h)
                f, ct = fmaps[i][l], tap_cotangents[i][l]
                if f is None:
                    raise ValueError(f"input_grad: feature map ({i}, {l}) is missing")
                if not f.is_cuda or f.dtype != torch.float32 or tuple(f.shape) != want or not f.is_contiguous():
                    raise ValueError(f"input_grad: feature map ({i}, {l}) must be a contiguous float32 device tensor of shape {want}: got {tuple(f.shape)}")
                if ct is not None:
                    if not (hasattr(ct, "is_cuda") and ct.is_cuda):
                        raise ValueError(f"input_grad: cotangent ({i}, {l}) must be a device tensor (there is no CPU path)")
                    if ct.numel() != f.numel() or int(ct.shape[0]) != B:
                        raise ValueError(f"input_grad: cotangent ({i}, {l}) must have the shape of its feature map {want}: got {tuple(ct.shape)}")
                    ct = ct.detach().to(torch.float32).contiguous()
                flat_f.append(f)
                flat_c.append(ct)
        work = [torch.empty_like(f) for f in flat_f]
        out = torch.empty(B, 1, T, dtype=torch.float32, device=dev)
        n = len(flat_f)
        pf = (C.c_void_p * n)(*[t.data_ptr() for t in flat_f])
        pc = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in flat_c])
        pw = (C.c_void_p * n)(*[t.data_ptr() for t in work])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.rvc_disc_input_grad(self._h, _lib.current_stream(), B, T, pf, pc, pw, _lib.ptr(out)))
        if return_deltas:
            it = iter(work)
            return out, [[next(it) for _ in rows] for rows in shapes]
        return out

    def weight_grad_launch_count(self, S, T):
        """Kernel launches of one weight_grad over S signals of T samples (rvc_disc_weight_grad_launch_count: the size of the plan; nothing is launched):
        two per layer (gradient, finish), whatever S and T."""
        n = _lib.lib.rvc_disc_weight_grad_launch_count(self._h, int(S), int(T))
        if n < 0:
            raise _lib.RvcHipError(_lib.lib.rvc_last_error().decode("utf-8", "replace"))
        return n

    def parameter_shapes(self):
        """OrderedDict name -> shape of the parameter tensors in the reference module's state-dict order (rvc_disc_param_info)."""
        assert self._loaded, "load_state_dict first"
        out = OrderedDict()
        name, shape, ndim = C.create_string_buffer(128), (_lib.c_int64 * 8)(), C.c_int()
        n = _lib.lib.rvc_disc_param_count(self._h)
        if n < 0:
            raise _lib.RvcHipError(_lib.lib.rvc_last_error().decode("utf-8", "replace"))
        for k in range(n):
            _lib.check(_lib.lib.rvc_disc_param_info(self._h, k, name, 128, shape, C.byref(ndim)))
            out[name.value.decode()] = tuple(int(shape[i]) for i in range(ndim.value))
        return out

    def weight_grad(self, x, fmaps, deltas):
        """The gradient with respect to every parameter (rvc_disc_weight_grad).  x [S,1,T]: the batch that produced `fmaps` (forward_single(x); for the
        trainer torch.cat([y, y_hat])); fmaps: those feature maps; deltas: what input_grad(fmaps, cotangents, return_deltas=True) returned beside the input
        gradient.  Returns an OrderedDict from state-dict name (per layer bias, weight_g, weight_v) to a float32 device tensor in the parameter's shape: views
        of ONE contiguous buffer in that order (`.flat` of the result holds it), so an optimizer can walk a single buffer.  Needs trainable=True."""
        assert self._loaded, "load_state_dict first"
        if not self.trainable:
            raise ValueError("weight_grad: the discriminators were built without trainable=True (weight_v / weight_g are not kept on the device)")
        if not (hasattr(x, "is_cuda") and x.is_cuda):
            raise ValueError("weight_grad: x must be a device tensor (there is no CPU path)")
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"weight_grad: x must be [S, 1, T]: got {tuple(x.shape)}")
        S_, T, dev = int(x.shape[0]), int(x.shape[2]), x.device
        for p in self.periods:
            if (p - T % p) % p >= T:
                raise ValueError(f"T = {T} is not longer than the reflect pad period {p} needs")
        shapes = self.tap_shapes(T)
        for what, lists in (("feature map", fmaps), ("delta", deltas)):
            if len(lists) != len(shapes) or [len(r) for r in lists] != [len(r) for r in shapes]:
                raise ValueError(f"weight_grad: one {what} per tap of every sub-discriminator expected")
        flat_f, flat_d = [], []
        for i, rows in enumerate(shapes):
            for l, (c, h, p) in enumerate(rows):
                want = (S_, c, h, p) if i else (S_, c, h)
                for what, t, dst in (("feature map", fmaps[i][l], flat_f), ("delta", deltas[i][l], flat_d)):
                    if t is None or not (hasattr(t, "is_cuda") and t.is_cuda) or t.device != dev:
                        raise ValueError(f"weight_grad: {what} ({i}, {l}) must be a tensor on {dev} (there is no CPU path)")
                    if t.dtype != torch.float32 or tuple(t.shape) != want or not t.is_contiguous():
                        raise ValueError(f"weight_grad: {what} ({i}, {l}) must be a contiguous float32 tensor of shape {want}: got {t.dtype} {tuple(t.shape)}")
                    dst.append(t)
        sig = x.detach().to(torch.float32).reshape(S_, T).contiguous()
        params = self.parameter_shapes()
        sizes = [int(np.prod(s)) for s in params.values()]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        out, o = _GradDict(), 0
        for (name, shape), n in zip(params.items(), sizes):
            out[name] = flat[o:o + n].view(shape)
            o += n
        out.flat = flat
        n = len(flat_f)
        pf = (C.c_void_p * n)(*[t.data_ptr() for t in flat_f])
        pd = (C.c_void_p * n)(*[t.data_ptr() for t in flat_d])
        pg = (C.c_void_p * len(out))(*[t.data_ptr() for t in out.values()])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.rvc_disc_weight_grad(self._h, _lib.current_stream(), _lib.ptr(sig), S_, T, pf, pd, pg))
        return out

    def _need_trainable(self, what):
        assert self._loaded, "load_state_dict first"
        if not self.trainable:
            raise ValueError(f"{what}: the discriminators were built without trainable=True (the parameters are not kept on the device)")

    def parameter_count(self):
        """Elements of all parameter tensors together: the length of weight_grad(...).flat and of the optimizer's state buffers."""
        self._need_trainable("parameter_count")
        with torch.cuda.device(self.device):
            n = _lib.lib.rvc_disc_param_total(self._h)
        if n < 0:
            raise _lib.RvcHipError(_lib.lib.rvc_last_error().decode("utf-8", "replace"))
        return int(n)

    def get_parameters(self):
        """The parameters the handle holds as ONE flat float32 device tensor in parameter_shapes() order (rvc_disc_get_parameters)."""
        self._need_trainable("get_parameters")
        flat = torch.empty(self.parameter_count(), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rvc_disc_get_parameters(self._h, _lib.current_stream(), _lib.ptr(flat)))
        return flat

    def load_parameters(self, flat):
        """Replaces every parameter from one flat float32 tensor in parameter_shapes() order and re-derives the folded weights and the weight images on
        the device (rvc_disc_set_parameters: the optimizer step's kernels, the bits rvc_disc_finalize would build)."""
        self._need_trainable("load_parameters")
        flat = torch.as_tensor(flat)
        if flat.dim() != 1 or flat.numel() != self.parameter_count():
            raise ValueError(f"load_parameters: a flat tensor of {self.parameter_count()} elements expected, got {tuple(flat.shape)}")
        flat = flat.detach().to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rvc_disc_set_parameters(self._h, _lib.current_stream(), _lib.ptr(flat)))
            torch.cuda.current_stream().synchronize()          # `flat` may be a temporary of this call
        return self

    def state_dict(self):
        """OrderedDict name -> host float32 tensor of every parameter as the handle holds it now, in parameter_shapes() order: what the reference module's
        state_dict() gives (trainable nets only: a frozen net keeps no parameters)."""
        self._need_trainable("state_dict")
        flat = self.get_parameters().cpu()
        out, o = OrderedDict(), 0
        for name, shape in self.parameter_shapes().items():
            n = int(np.prod(shape))
            out[name] = flat[o:o + n].view(shape).clone()
            o += n
        return out

    def adamw_step_launch_count(self):
        """Kernel launches of one optimizer step (rvc_disc_adamw_step_launch_count): a constant of the net."""
        self._need_trainable("adamw_step_launch_count")
        with torch.cuda.device(self.device):
            n = _lib.lib.rvc_disc_adamw_step_launch_count(self._h)
        if n < 0:
            raise _lib.RvcHipError(_lib.lib.rvc_last_error().decode("utf-8", "replace"))
        return n

    def adamw_step(self, grads_flat, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, step, clip_value=None):
        """One AdamW step on the parameters the handle holds (rvc_disc_adamw_step); lib.train.optim.AdamW is the public face.  The three flat float32
        device tensors are in parameter_shapes() order; exp_avg / exp_avg_sq are updated in place, grads_flat is only read."""
        self._need_trainable("adamw_step")
        n = self.parameter_count()
        for what, t in (("grads", grads_flat), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            if not (hasattr(t, "is_cuda") and t.is_cuda) or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
                raise ValueError(f"adamw_step: {what} must be a contiguous flat float32 device tensor of {n} elements")
        h = _lib.AdamwHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), int(clip_value is not None),
                            float(clip_value) if clip_value is not None else 0.0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rvc_disc_adamw_step(self._h, _lib.current_stream(), _lib.ptr(grads_flat), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), C.byref(h)))

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


class _GradDict(OrderedDict):
    """weight_grad's result: name -> gradient view; `.flat` is the one contiguous float32 buffer the views share, in the dict's order."""
    flat = None


class MultiPeriodDiscriminator(_MultiPeriodDiscriminator):
    """v1: periods 2, 3, 5, 7, 11, 17 (reference lib/infer_pack/models.py:1024-1049)."""
    VERSION = 1


class MultiPeriodDiscriminatorV2(_MultiPeriodDiscriminator):
    """v2: periods 2, 3, 5, 7, 11, 17, 23, 37 (reference lib/infer_pack/models.py:1052-1079)."""
    VERSION = 2

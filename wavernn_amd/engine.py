"""LoopEngine: the Python face of the C ABI for the autoregressive loop (include/wavernn_amd.h).

PyTorch is used only for device memory and streams; all computation happens in libwavernn_amd.so.
"""
import ctypes
import numpy as np
import torch

from . import _lib

LOOP_KEYS = dict(I_w='I.weight', I_b='I.bias', w_ih1='rnn1.weight_ih_l0', w_hh1='rnn1.weight_hh_l0',
                 b_ih1='rnn1.bias_ih_l0', b_hh1='rnn1.bias_hh_l0', w_ih2='rnn2.weight_ih_l0', w_hh2='rnn2.weight_hh_l0',
                 b_ih2='rnn2.bias_ih_l0', b_hh2='rnn2.bias_hh_l0', fc1_w='fc1.weight', fc1_b='fc1.bias',
                 fc2_w='fc2.weight', fc2_b='fc2.bias', fc3_w='fc3.weight', fc3_b='fc3.bias')


#: loop kernels that keep their state between launches: a call can be continued in step slices (wrnn_options.t_begin / t_end).  The other models stream
#: through WATCHABLE_KERNELS: the call runs whole and says how far it has got (`run_segments(watch=...)`, `generate_unbatched(live=True)`)
RESUMABLE_KERNELS = ('wrnn_loop_kernel', 'wrnn_duo_kernel', 'wrnn_sparse_kernel', 'wrnn_chain_kernel')
#: loop kernels that are launched once for all steps and can publish their progress while they run (wrnn_generate_segments_watched)
WATCHABLE_KERNELS = ('wrnn_generic_kernel', 'wrnn_tile_kernel', 'wrnn_tile_sparse_kernel', 'wrnn_tile_bf16_kernel', 'wrnn_tile_wide_kernel')
#: ... and those that form the last up-sampling stage of the mel themselves (wrnn_options.mel_stage: they take `MelRows`)
MEL_STAGE_KERNELS = ('wrnn_duo_kernel', 'wrnn_sparse_kernel', 'wrnn_chain_kernel')
#: the persistent kernels: kernel -> (the algo that asks for it by name, what `auto` falls back to when its grid is refused -- cooperative launch not
#: co-resident; None: the stream kernel)
KERNEL_ALGOS = {'wrnn_sparse_kernel': ('sparse', 'duo'), 'wrnn_chain_kernel': ('chain', 'duo'), 'wrnn_octo_kernel': ('octo', 'duo'),
                'wrnn_duo_kernel': ('duo', 'loop'), 'wrnn_loop_kernel': ('loop', None)}
FALLBACK_ALGO = {k: nxt for k, (_, nxt) in KERNEL_ALGOS.items() if nxt}


class MelRows:
    """The conditioning mel handed to the loop ONE up-sampling stage short (`wrnn_options.mel_stage = 1`; wrnn_duo_kernel, wrnn_chain_kernel and wrnn_sparse_kernel): the
    kernel forms the last Stretch2d + conv stage and the crop (reference models/fatchord_version.py:73-80, :86-88) itself, so the
    [L, feat] up-sampled mel is never written.

    rows      (n_rows, feat) float32 CUDA tensor: `PreEngine.upsample_rows` output (several utterances: their blocks one after the other)
    L         length of the cropped time line the segment table refers to (what `mels_up.shape[0]` would have been)
    scale     stretch factor of the last stage; taps: its 2 * scale + 1 conv taps (host)
    seg_off   un-cropped position of step t of segment b = seg_pos[b] + t + seg_off[b]: one int, or one per segment
              (utterance k of a concatenation: indent * (2 k + 1), indent = pad * hop)"""

    def __init__(self, rows, L, scale, taps, seg_off):
        self.rows, self.L, self.scale = rows, int(L), int(scale)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.seg_off = seg_off
        if self.taps.shape[0] != 2 * self.scale + 1:
            raise ValueError('the last stage has 2 * scale + 1 taps')

    @property
    def shape(self):
        return self.rows.shape


def _as_host_f32(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().to('cpu', torch.float32).numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


class LoopEngine:
    """Device-resident weight pack + `run()` = one call of `wrnn_generate`.

    state_dict: mapping with the reference's loop keys (LOOP_KEYS values), torch tensors or numpy arrays.
    """

    def __init__(self, state_dict, mode, device=None):
        if not torch.cuda.is_available():
            raise _lib.WrnnError('wavernn_amd needs a HIP device (torch.cuda.is_available() is False); '
                                 'there is no CPU fallback')
        self.lib = _lib.lib()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.mode = mode
        host = {k: _as_host_f32(state_dict[v]) for k, v in LOOP_KEYS.items()}
        w = _lib.Weights()
        w.rnn_dims = host['w_hh1'].shape[1]
        w.fc_dims = host['fc1_w'].shape[0]
        w.aux_dims = host['w_ih2'].shape[1] - w.rnn_dims
        w.feat_dims = host['I_w'].shape[1] - 1 - w.aux_dims
        w.n_classes = host['fc3_w'].shape[0]
        if mode not in ('RAW', 'MOL'):
            raise RuntimeError("Unknown model mode value - ", mode)
        w.mode = _lib.MODE_MOL if mode == 'MOL' else _lib.MODE_RAW
        for k, a in host.items():
            setattr(w, k, a.ctypes.data)
        self.n_classes = int(w.n_classes)
        self.feat_dims, self.aux_dims = int(w.feat_dims), int(w.aux_dims)
        pack = ctypes.c_void_p()
        _lib.check(self.lib.wrnn_pack_create(ctypes.byref(w), self._dev_index, ctypes.byref(pack)), 'wrnn_pack_create')
        self._pack = pack
        self._ws = None
        self.n_cus = self.lib.wrnn_device_cus(self._dev_index)
        # a pruned 9-bit model: `auto` runs its masked weights on the dense kernels (their summation order is the oracle's); the block-sparse kernel's
        # RAW mode runs on request -- say so once instead of choosing silently
        if mode == 'RAW' and min(float(np.count_nonzero(host[k])) / host[k].size for k in ('w_ih1', 'w_hh1', 'w_ih2', 'w_hh2')) < 0.5:
            import warnings
            warnings.warn("wavernn_amd: this 9-bit RAW model has pruned GRU matrices; algo='auto' runs the masked weights on the dense kernels (the "
                          "dense step time); model.loop_algo = 'sparse' / algo='sparse' runs the block-sparse loop kernel (wrnn_sparse_kernel)")
        timer = ctypes.c_void_p()
        _lib.check(self.lib.wrnn_timer_create(self._dev_index, ctypes.byref(timer)), 'wrnn_timer_create')
        self._timer = timer
        self._info = _lib.RunInfo()
        self._last_opts = None
        self._launches = 0
        self._slice_algo = None
        self._auto_floor = None           # the kernel an `auto` call degraded to after a refused cooperative launch: where later `auto` calls start
        #: workgroups per tile (2, 4, 8) of an algo='tile' call that names no `clusters` itself: wrnn_tile_wide_kernel (`WaveRNN.tile_width` sets it).  A call
        #: with more segments than the width takes on this device, or whose cooperative launch is refused, runs on plain wrnn_tile_kernel: one warning
        self.tile_width = 0
        self._tile_narrow = False         # a wide launch was refused (not co-resident): later calls stay on wrnn_tile_kernel
        self._tile_warned = False
        self._progress_keep = []          # ctypes thunks of progress callbacks whose host functions may still be queued on the stream

    def __del__(self):
        try:
            if getattr(self, '_timer', None):
                self.lib.wrnn_timer_destroy(self._timer)
                self._timer = None
            if getattr(self, '_pack', None):
                self.lib.wrnn_pack_destroy(self._pack)
                self._pack = None
        except Exception:
            pass

    @property
    def sparse_blocks(self):
        """> 0: the block-sparse kernel can run this pack (largest block-row population); <= 0: it cannot."""
        return int(self.lib.wrnn_pack_sparse_blocks(self._pack))

    @property
    def sparse_fc_blocks(self):
        """> 0: fc1 / fc2 are block-sparse too (the notebook's recipe prunes the Linear layers) -> the sparse kernel's gathered fc stages."""
        return int(self.lib.wrnn_pack_sparse_fc_blocks(self._pack))

    def tile_sparse_view(self):
        """(view, kept, total) of `wrnn_pack_tile_sparse`: view 0 -- algo='tile_sparse' refuses this pack --, 1 (the GRU matrices run on their surviving 16x1
        blocks) or 2 (fc1 / fc2 too); kept / total: surviving and all blocks of rnn1 ih, rnn1 hh, rnn2 ih, rnn2 hh, fc1, fc2."""
        kept, total = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
        view = int(self.lib.wrnn_pack_tile_sparse(self._pack, ctypes.byref(kept), ctypes.byref(total)))
        return view, [int(k) for k in kept], [int(t) for t in total]

    def tile_bf16_bytes(self):
        """`wrnn_pack_tile_bf16`: bytes of the pack's bf16 view; 0 -- algo='tile_bf16' refuses this pack: the shipped dims, dims past wrnn_tile_kernel's
        LDS rule, or a weight that rounds to +-inf in bfloat16."""
        return int(self.lib.wrnn_pack_tile_bf16(self._pack))

    @property
    def weight_bytes(self):
        return int(self.lib.wrnn_pack_weight_bytes(self._pack))

    def run(self, mels_up, aux, B, T, stride, noise, hop, **kw):
        """One utterance: segment b reads conditioning position b*stride + t (`fold_with_overlap` geometry,
        reference :293-340; unbatched: B=1, T=L, stride=0).  See `run_segments`."""
        L = mels_up.L if isinstance(mels_up, MelRows) else mels_up.shape[0]
        seg_pos = np.arange(B, dtype=np.int32) * np.int32(stride)
        seg_lim = np.full(B, L, dtype=np.int32)
        return self.run_segments(mels_up, aux, seg_pos, seg_lim, T, noise, hop, **kw)

    def options(self, algo='auto', depth=0, clusters=0, slab_steps=0, cond_valu=False, t_range=None, tuning=0, sparse_groups=0, noise_lib=False):
        if algo == 'auto' and self._auto_floor is not None:      # (after a refused cooperative launch: see run_segments)
            algo = self._auto_floor
        o = _lib.Options()
        o.algo = _lib.ALGOS[algo]
        o.depth, o.clusters, o.slab_steps, o.cond_valu = int(depth), int(clusters), int(slab_steps), int(bool(cond_valu))
        o.tuning = int(tuning)
        o.sparse_groups = int(sparse_groups or 0)      # wrnn_sparse_kernel: 2 = two groups per cluster (on request; any other kernel refuses it)
        o.noise_lib = int(bool(noise_lib))             # the library draws the sampling noise (a slab of it joins the workspace; may shorten a RAW slab)
        if t_range is not None:
            o.t_begin, o.t_end = int(t_range[0]), int(t_range[1])
        return o

    def _tile_clusters(self, algo, clusters, n_segments, T):
        """`clusters` of a call: under algo='tile' with none named, `self.tile_width` where the planner takes this many segments at that width."""
        if algo != 'tile' or clusters or self.tile_width <= 1 or self._tile_narrow:
            return clusters
        o, i = self.options('tile', clusters=self.tile_width), _lib.RunInfo()
        rc = self.lib.wrnn_plan_segments(self._pack, n_segments, T, ctypes.byref(o), ctypes.byref(i))
        why = self.lib.wrnn_last_error().decode()
        if rc == _lib.ERR_ARG and 'takes at most' in why:       # too many segments for this width: the planner's own answer names plain tile
            self._warn_tile(why)
            return 0
        return self.tile_width                                  # (any other refusal is the call's own to raise)

    def _warn_tile(self, why):
        if not self._tile_warned:
            import warnings
            warnings.warn('wavernn_amd: ' + why + '; running on wrnn_tile_kernel (tile_width ignored for such calls)')
            self._tile_warned = True

    def plan(self, n_segments, T, **kw):
        """What a run over this many segments would launch (`wrnn_plan_segments`): dict(kernel, clusters, depth, rounds, ...)."""
        kw['clusters'] = self._tile_clusters(kw.get('algo', 'auto'), kw.get('clusters', 0), n_segments, T)
        o, i = self.options(**kw), _lib.RunInfo()
        _lib.check(self.lib.wrnn_plan_segments(self._pack, n_segments, T, ctypes.byref(o), ctypes.byref(i)), 'wrnn_plan_segments')
        return dict(kernel=(i.kernel or b'').decode(), units_per_wg=int(i.units_per_wg), clusters=int(i.clusters), depth=int(i.depth),
                    rounds=int(i.rounds), slab_steps=int(i.slab_steps))

    def workspace_bytes(self, n_segments, T, n_frames, **kw):
        kw['clusters'] = self._tile_clusters(kw.get('algo', 'auto'), kw.get('clusters', 0), n_segments, T)
        o = self.options(**kw)
        return int(self.lib.wrnn_workspace_bytes_segments(self._pack, n_segments, T, n_frames, ctypes.byref(o)))

    def watch_words(self, n_segments, T, algo='auto', clusters=0):
        """`wrnn_watch_words`: the progress words a watched call over this many segments writes (one per workgroup that writes `out`); raises WrnnError
        with the library's reason when the call would not run on one of WATCHABLE_KERNELS."""
        o, words = self.options(algo, clusters=self._tile_clusters(algo, clusters, n_segments, T)), ctypes.c_int32(0)
        _lib.check(self.lib.wrnn_watch_words(self._pack, n_segments, T, ctypes.byref(o), ctypes.byref(words)), 'wrnn_watch_words')
        return int(words.value)

    def run_segments(self, mels_up, aux, seg_pos, seg_lim, T, noise, hop, algo='auto', force_x=None, want_logits=False,
                     check=True, depth=0, clusters=0, slab_steps=0, cond_valu=False, t_range=None, out=None, logits=None,
                     phase_clocks=None, tuning=0, progress=None, sparse_groups=0, noise_seed=0, noise_seg_id=None, watch=None, _fallback=False):
        """mels_up (L,feat) / aux (n_frames,4*aux_dims) / noise: float32 CUDA tensors; seg_pos / seg_lim: host
        int32 arrays (B,) -- segment b, step t reads position seg_pos[b]+t, zero conditioning from seg_lim[b] on
        (several utterances: concatenated conditioning).  Returns out (B,T) CUDA [and logits (T,B,C)].
        Enqueues on the current stream; `check=True` synchronises and raises if a kernel gave up.

        depth / clusters / slab_steps / cond_valu / sparse_groups: `wrnn_options` (0 = the library picks; sparse_groups=2: two groups per
        cluster of wrnn_sparse_kernel, same samples; algo='tile': clusters = 2, 4, 8 runs wrnn_tile_wide_kernel, that many workgroups per tile of 16
        segments, same samples -- none named: `self.tile_width`).  t_range=(t0, t1) runs only those
        steps; t0 > 0 continues the previous call on this engine's workspace (pass the same `out`; `noise` then holds the
        rows of [t0, t1) only) -- how long RAW runs draw their noise in chunks instead of T*B*C floats at once.
        progress: optional `f(steps_done, T, n_segments)` called from a HIP runtime thread when the device has finished each
        conditioning slab (wrnn_options.progress; must not touch the device).
        noise=None: the library draws the noise itself (wrnn_options.noise_lib), slab by slab on the stream, from the counter-based generator
        keyed by `noise_seed`; noise_seg_id: one 64-bit stream id per segment (None: segment b has id b).  The samples are those of the same
        call fed `rng.library_noise(...)`; a continued call (t_range) needs nothing but the same seed and ids.
        watch=(words, every): a WATCHED call (`wrnn_generate_segments_watched`; a kernel of WATCHABLE_KERNELS, whole calls only -- anything else raises):
        `words` is a uint32 (or int32) CUDA tensor of at least `watch_words(...)` elements that the caller has zeroed on this stream; after every `every`
        steps each workgroup that writes `out` stores the steps it has finished into its word, so min(words[:watch_words]) = the columns of `out` that a
        kernel or copy launched from then on may read.  Same samples as the plain call."""
        rows_in = mels_up if isinstance(mels_up, MelRows) else None
        if rows_in is not None:
            mels_up = rows_in.rows
        lib_noise = noise is None
        for name, t_ in (('mels_up', mels_up), ('aux', aux)) + (() if lib_noise else (('noise', noise),)):
            if not (t_.is_cuda and t_.dtype == torch.float32 and t_.is_contiguous()):
                raise ValueError(f'{name} must be a contiguous float32 CUDA tensor')
        seg_pos = np.ascontiguousarray(seg_pos, dtype=np.int32)
        seg_lim = np.ascontiguousarray(seg_lim, dtype=np.int32)
        B = int(seg_pos.shape[0])
        if seg_lim.shape != (B,) or B < 1:
            raise ValueError('seg_pos / seg_lim must be 1-D int32 arrays of equal, non-zero length')
        L = rows_in.L if rows_in is not None else mels_up.shape[0]
        if mels_up.shape[1] != self.feat_dims or aux.shape[1] != 4 * self.aux_dims:
            raise ValueError('conditioning shape mismatch')
        t0, t1 = (0, T) if t_range is None else (int(t_range[0]), int(t_range[1]))
        if t0 > 0 and algo == 'auto' and self._slice_algo is not None:
            # a continuation runs on the kernel its first slice settled on (`auto` may have fallen back from two workgroups per CU to
            # one on that slice only; the two kernels keep different state / ring layouts -- the library also checks: status word 8)
            algo = self._slice_algo
        need = (t1 - t0) * 11 * B if self.mode == 'MOL' else (t1 - t0) * B * self.n_classes
        if not lib_noise and noise.numel() != need:
            raise ValueError(f'noise has {noise.numel()} elements, expected {need}')
        n_frames = int(aux.shape[0])
        named_clusters = clusters
        clusters = self._tile_clusters(algo, clusters, B, T)
        o = self.options(algo, depth, clusters, slab_steps, cond_valu, t_range, tuning, sparse_groups, lib_noise)
        if lib_noise:                     # (the id array is a host array read during the call only)
            o.noise_seed = int(noise_seed) & (2 ** 64 - 1)
            if noise_seg_id is not None:
                noise_seg_id = np.ascontiguousarray(noise_seg_id, dtype=np.uint64)
                if noise_seg_id.shape != (B,):
                    raise ValueError('noise_seg_id: one 64-bit id per segment')
                o.noise_seg_id = noise_seg_id.ctypes.data
        nbytes = int(self.lib.wrnn_workspace_bytes_segments(self._pack, B, T, n_frames, ctypes.byref(o)))
        if nbytes == 0:
            raise _lib.WrnnError('bad geometry / options: ' + self.lib.wrnn_last_error().decode())
        if self._ws is None or self._ws.numel() < nbytes:
            if t0 > 0:
                raise _lib.WrnnError('continuing a call needs the workspace of the call it continues')
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty(B, T, dtype=torch.float32, device=self.device)
        if force_x is not None:
            force_x = force_x.to(self.device, torch.float32).contiguous()
            assert force_x.shape == (B, T)
            o.force_x = force_x.data_ptr()
        if want_logits:
            if logits is None:
                logits = torch.empty(T, B, self.n_classes, dtype=torch.float32, device=self.device)
            o.logits = logits.data_ptr()
        if phase_clocks is not None:      # profiling hook: int64 CUDA tensor [256, 32], zeroed by the caller
            o.phase_clocks = phase_clocks.data_ptr()
        if progress is not None:          # the thunk must outlive the host functions queued behind the slabs: released after a synchronisation
            thunk = _lib.PROGRESS_FN(lambda done, T_, n_, user: progress(int(done), int(T_), int(n_)))
            self._progress_keep.append(thunk)
            o.progress = ctypes.cast(thunk, ctypes.c_void_p)
        o.timer = self._timer
        o.info = ctypes.pointer(self._info)
        if rows_in is not None:           # (host arrays read during the call only)
            seg_moff = np.ascontiguousarray(np.broadcast_to(np.asarray(rows_in.seg_off, dtype=np.int32), (B,)))
            o.mel_stage, o.mel_rows, o.mel_scale = 1, int(mels_up.shape[0]), rows_in.scale
            o.mel_taps, o.seg_moff = rows_in.taps.ctypes.data, seg_moff.ctypes.data
        stream = torch.cuda.current_stream(self.device).cuda_stream
        call_args = (self._pack, B, T, seg_pos.ctypes.data, seg_lim.ctypes.data, L, hop, n_frames,
                     mels_up.data_ptr(), aux.data_ptr(), None if lib_noise else noise.data_ptr(), out.data_ptr(),
                     self._ws.data_ptr(), self._ws.numel(), ctypes.byref(o), stream)
        if watch is None:
            rc = self.lib.wrnn_generate_segments(*call_args)
        else:
            words, every = watch
            if not (words.is_cuda and words.dtype in (torch.uint32, torch.int32) and words.is_contiguous()):
                raise ValueError('watch: (a contiguous uint32 CUDA tensor, steps between two publications)')
            rc = self.lib.wrnn_generate_segments_watched(*call_args, words.data_ptr(), int(words.numel()), int(every))
        if rc == _lib.ERR_RESIDENCY and algo == 'tile' and clusters > 1 and not named_clusters:
            # the W workgroups of a tile are not co-resident right now: plain wrnn_tile_kernel needs no residency (the same samples), from now on
            self._warn_tile('cooperative launch refused (' + self.lib.wrnn_last_error().decode() + ')')
            self._tile_narrow = True
            if progress is not None:
                self._progress_keep.pop()
            return self.run_segments(mels_up if rows_in is None else rows_in, aux, seg_pos, seg_lim, T, noise, hop, algo=algo, force_x=force_x,
                                     want_logits=want_logits, check=check, slab_steps=slab_steps, cond_valu=cond_valu, t_range=t_range, out=out, logits=logits,
                                     phase_clocks=phase_clocks, tuning=tuning, progress=progress, noise_seed=noise_seed, noise_seg_id=noise_seg_id, watch=watch)
        if rc == _lib.ERR_RESIDENCY and t0 == 0 and (algo == 'auto' or _fallback):
            # the persistent grid is not co-resident right now (CU masking, a smaller partition, another cooperative kernel).  `auto`
            # degrades step by step (FALLBACK_ALGO): wrnn_sparse_kernel -> two workgroups per CU (wrnn_duo_kernel) -> one (wrnn_loop_kernel;
            # each has its own workspace layout, continuations are pinned to the kernel the first slice ran on) -> the stream kernel (any
            # device, no inter-workgroup traffic; whole calls only).  sparse_groups is a speed hint for wrnn_sparse_kernel: the next kernel runs without it
            import warnings
            why = self.lib.wrnn_last_error().decode()
            planned = _lib.RunInfo()
            self.lib.wrnn_plan_segments(self._pack, B, T, ctypes.byref(o), ctypes.byref(planned))
            nxt = FALLBACK_ALGO.get((planned.kernel or b'').decode())
            if rows_in is not None and nxt != 'duo':       # the other kernels read the up-sampled mel: the caller, who has the mel, redoes the conditioning
                raise _lib.ResidencyError('cooperative launch refused (' + why + ')')
            if rows_in is not None:
                mels_up = rows_in
            if nxt is not None:
                warnings.warn('wavernn_amd: cooperative launch refused (' + why + '); trying algo = ' + nxt)
                self._ws = None
                if progress is not None:
                    self._progress_keep.pop()       # (the retry registers its own thunk)
                res = self.run_segments(mels_up, aux, seg_pos, seg_lim, T, noise, hop, algo=nxt, depth=depth, clusters=clusters, force_x=force_x,
                                        want_logits=want_logits, check=check, slab_steps=slab_steps, cond_valu=cond_valu, t_range=t_range, out=out,
                                        logits=logits, phase_clocks=phase_clocks, tuning=tuning, progress=progress, noise_seed=noise_seed, noise_seg_id=noise_seg_id, _fallback=True)      # (sparse_groups: wrnn_sparse_kernel's alone -- dropped)
                if algo == 'auto':
                    self._auto_floor = self._auto_floor or nxt       # later `auto` calls start from the kernel that ran (no refused launch + workspace re-allocation per call)
                return res
            if t1 == T:
                warnings.warn('wavernn_amd: cooperative launch refused (' + why + '); using the stream kernel')
                if progress is not None:
                    self._progress_keep.pop()
                if algo == 'auto':
                    self._auto_floor = 'stream'
                return self.run_segments(mels_up, aux, seg_pos, seg_lim, T, noise, hop, algo='stream', force_x=force_x,
                                         want_logits=want_logits, check=check, slab_steps=slab_steps, cond_valu=cond_valu, out=out, logits=logits,
                                         phase_clocks=phase_clocks, tuning=tuning, progress=progress, noise_seed=noise_seed, noise_seg_id=noise_seg_id)
            # ... the same refusal on the first slice of a step-sliced run (only the loop kernels continue a call): the caller, who owns
            # the slicing and the noise stream, redoes the whole call on the stream kernel
            raise _lib.ResidencyError('cooperative launch refused (' + why + ')')
        _lib.check(rc, 'wrnn_generate_segments' if watch is None else 'wrnn_generate_segments_watched')
        self._launches = (self._launches if t0 > 0 else 0) + int(self._info.launches)
        if t0 == 0:
            self._slice_algo = KERNEL_ALGOS.get((self._info.kernel or b'').decode(), (None, None))[0]
        self._last_opts = (B, T, n_frames, self.options(algo, depth, clusters, slab_steps, cond_valu, None, 0, sparse_groups, lib_noise))
        if check:
            rc = self.lib.wrnn_status(self._ws.data_ptr(), stream)      # synchronises the stream: every queued progress call has run
            del self._progress_keep[:]
            _lib.check(rc, 'loop kernel')
        return (out, logits) if want_logits else out

    def status(self):
        """Synchronise the current stream and raise if a loop kernel of the last call gave up (for `check=False` calls)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.wrnn_status(self._ws.data_ptr(), stream)
        del self._progress_keep[:]
        _lib.check(rc, 'loop kernel')

    def read_exchange(self, cluster, slot, layer, ring):
        """Test hook: one exchanged layer (0 h1, 1 h2, 2 y1, 3 y2, 4 RAW logits) of the last loop-kernel call as a host
        array [16 segments, 512] (wrnn_debug_read_exchange)."""
        B, T, n_frames, o = self._last_opts
        host = np.zeros((16, 512), np.float32)
        _lib.check(self.lib.wrnn_debug_read_exchange(self._pack, self._ws.data_ptr(), B, T, n_frames, ctypes.byref(o), cluster,
                                                     slot, layer, ring, host.ctypes.data), 'wrnn_debug_read_exchange')
        return host

    def last_loop_split(self):
        """(hidden units per workgroup, independent clusters, groups in flight per cluster) of the last call;
        (0, 0, 0) for the stream kernel."""
        i = self._info
        return int(i.units_per_wg), int(i.clusters), int(i.depth)

    def last_run_info(self):
        i = self._info
        return dict(kernel=(i.kernel or b'').decode(), units_per_wg=int(i.units_per_wg), clusters=int(i.clusters), depth=int(i.depth),
                    rounds=int(i.rounds), slab_steps=int(i.slab_steps), launches=int(self._launches))

    def last_loop_ms(self):
        """Sum of the loop-kernel launch durations of the last call, continuations (t_range with t0 > 0) included (HIP events on
        the launch stream; synchronises)."""
        return float(self.lib.wrnn_timer_ms(self._timer))

    def last_loop_kernel(self):
        return (self._info.kernel or b'').decode()

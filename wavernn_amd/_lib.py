"""ctypes binding of libwavernn_amd.so (the C ABI declared in include/wavernn_amd.h).

The library holds the HIP kernels; there is NO CPU fallback.  If the shared object is missing, or no HIP
device is present, the product path raises -- loudly -- instead of computing anything on the host.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
SO_PATH = os.path.join(CSRC, 'libwavernn_amd.so')

WRNN_OK = 0
ERR_ARG = -1                # WRNN_ERR_ARG: bad argument / unsupported dims
ERR_NO_DEVICE = -2          # WRNN_ERR_NO_DEVICE
ERR_RESIDENCY = -6          # WRNN_ERR_RESIDENCY: the persistent grid cannot be co-resident on this device
MODE_RAW, MODE_MOL = 0, 1
ABI_VERSION = 9
ALGO_AUTO, ALGO_STREAM, ALGO_LOOP, ALGO_SPARSE, ALGO_DUO, ALGO_CHAIN, ALGO_OCTO, ALGO_TILE, ALGO_TILE_SPARSE, ALGO_TILE_BF16 = 0, 1, 2, 5, 6, 7, 8, 10, 12, 13
ALGOS = {'auto': ALGO_AUTO, 'stream': ALGO_STREAM, 'loop': ALGO_LOOP, 'sparse': ALGO_SPARSE, 'duo': ALGO_DUO, 'chain': ALGO_CHAIN, 'octo': ALGO_OCTO, 'tile': ALGO_TILE,
         'tile_sparse': ALGO_TILE_SPARSE, 'tile_bf16': ALGO_TILE_BF16}

#: every symbol include/wavernn_amd.h declares
EXPORTS = ['wrnn_last_error', 'wrnn_abi_version', 'wrnn_device_cus', 'wrnn_pack_create', 'wrnn_pack_destroy',
           'wrnn_pack_weight_bytes', 'wrnn_pack_sparse_blocks', 'wrnn_pack_sparse_fc_blocks', 'wrnn_pack_tile_sparse', 'wrnn_pack_tile_bf16', 'wrnn_debug_tile_bf16_pack', 'wrnn_debug_tile_sparse_pack', 'wrnn_workspace_bytes', 'wrnn_workspace_bytes_segments', 'wrnn_generate',
           'wrnn_generate_segments', 'wrnn_noise_fill', 'wrnn_noise_fill_host', 'wrnn_nll', 'wrnn_nll_host', 'wrnn_plan_segments', 'wrnn_status', 'wrnn_timer_create', 'wrnn_timer_destroy', 'wrnn_timer_ms',
           'wrnn_timer_launches', 'wrnn_debug_read_exchange', 'wrnn_debug_plan', 'wrnn_selftest', 'wrnn_selftest_metric', 'wrnn_pre_create',
           'wrnn_pre_destroy', 'wrnn_pre_hop', 'wrnn_pre_workspace_bytes', 'wrnn_pre_upsample', 'wrnn_pre_upsample_rows', 'wrnn_pre_workspace_bytes_many',
           'wrnn_pre_upsample_many', 'wrnn_pre_debug_host_handle', 'wrnn_pre_last_error',
           'wrnn_post_unfold', 'wrnn_post_last_error', 'wrnn_post_chunk', 'wrnn_post_chunk_host', 'wrnn_taco_workspace_bytes', 'wrnn_taco_decode', 'wrnn_taco_status',
           'wrnn_taco_last_error', 'wrnn_bigru', 'wrnn_taco_front_create', 'wrnn_taco_front_destroy', 'wrnn_taco_front_workspace_bytes',
           'wrnn_taco_encode', 'wrnn_taco_postnet', 'wrnn_taco_batch_workspace_bytes', 'wrnn_taco_decode_batch',
           'wrnn_bigru_many', 'wrnn_taco_front_workspace_bytes_many', 'wrnn_taco_encode_many', 'wrnn_taco_postnet_many',
           'wrnn_taco_front_debug_host_handle', 'wrnn_taco_forced_workspace_bytes', 'wrnn_taco_decode_forced',
           'wrnn_taco_decode_batch_groups', 'wrnn_taco_decode_forced_groups', 'wrnn_debug_taco_group_of',
           'wrnn_generate_segments_watched', 'wrnn_watch_words', 'wrnn_debug_watch']


class Weights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('rnn_dims', 'fc_dims', 'feat_dims', 'aux_dims', 'n_classes', 'mode')] + \
               [(n, ctypes.c_void_p) for n in ('I_w', 'I_b', 'w_ih1', 'w_hh1', 'b_ih1', 'b_hh1', 'w_ih2', 'w_hh2',
                                               'b_ih2', 'b_hh2', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'fc3_w', 'fc3_b')]


class PreWeights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('feat_dims', 'compute_dims', 'res_out_dims', 'res_blocks', 'pad')] + \
               [('upsample_factors', ctypes.c_int32 * 3)] + \
               [(n, ctypes.c_void_p) for n in ('conv_in_w', 'bn_in', 'res_w', 'res_bn', 'conv_out_w', 'conv_out_b', 'up_w')]


class PreUtt(ctypes.Structure):
    """wrnn_pre_utt: one utterance of a `wrnn_pre_upsample_many` table."""
    _fields_ = [('mel', ctypes.c_void_p), ('n_frames', ctypes.c_int32), ('reserved', ctypes.c_int32), ('up_row', ctypes.c_int64),
                ('aux_row', ctypes.c_int64)]


TACO_WEIGHT_FIELDS = ('prenet_fc1_w', 'prenet_fc1_b', 'prenet_fc2_w', 'prenet_fc2_b', 'attn_rnn_w_ih', 'attn_rnn_w_hh', 'attn_rnn_b_ih',
                      'attn_rnn_b_hh', 'attn_W_w', 'attn_W_b', 'attn_conv_w', 'attn_L_w', 'attn_L_b', 'attn_v_w', 'rnn_input_w', 'rnn_input_b',
                      'rnn1_w_ih', 'rnn1_w_hh', 'rnn1_b_ih', 'rnn1_b_hh', 'rnn2_w_ih', 'rnn2_w_hh', 'rnn2_b_ih', 'rnn2_b_hh', 'mel_proj_w')


class TacoWeights(ctypes.Structure):
    """wrnn_taco_weights (the Tacotron decoder kernels)."""
    _fields_ = [('struct_bytes', ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ('n_mels', 'prenet1', 'prenet2', 'decoder_dims', 'encoder_width', 'lstm_dims', 'attn_filters',
                                              'attn_kernel')] + \
               [(n, ctypes.c_void_p) for n in TACO_WEIGHT_FIELDS]


class TacoCall(ctypes.Structure):
    """wrnn_taco_call."""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('n', ctypes.c_int32), ('r', ctypes.c_int32), ('max_r', ctypes.c_int32),
                ('max_steps', ctypes.c_int32), ('stop_threshold', ctypes.c_float), ('seq', ctypes.c_void_p), ('seq_proj', ctypes.c_void_p),
                ('mel_out', ctypes.c_void_p), ('scores_out', ctypes.c_void_p), ('steps_done', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p), ('variant', ctypes.c_int32)]


TACO_BATCH_MAX = 8           # WRNN_TACO_BATCH_MAX: sentences per wrnn_taco_decode_batch call
TACO_BATCH_NMAX = 256        # WRNN_TACO_BATCH_NMAX: encoder positions per sentence in that call
TACO_GROUPS_MAX = 2          # WRNN_TACO_GROUPS_MAX: sentence groups per wrnn_taco_decode_batch_groups / wrnn_taco_decode_forced_groups call


class TacoBatchCall(ctypes.Structure):
    """wrnn_taco_batch_call: n / max_steps / seq / seq_proj / mel_out / scores_out point to HOST arrays of n_sent entries."""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('n_sent', ctypes.c_int32), ('r', ctypes.c_int32), ('max_r', ctypes.c_int32),
                ('stop_threshold', ctypes.c_float), ('n', ctypes.POINTER(ctypes.c_int32)), ('max_steps', ctypes.POINTER(ctypes.c_int32)),
                ('seq', ctypes.POINTER(ctypes.c_void_p)), ('seq_proj', ctypes.POINTER(ctypes.c_void_p)),
                ('mel_out', ctypes.POINTER(ctypes.c_void_p)), ('scores_out', ctypes.POINTER(ctypes.c_void_p)),
                ('steps_done', ctypes.c_void_p), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t), ('stream', ctypes.c_void_p)]


class TacoForcedCall(ctypes.Structure):
    """wrnn_taco_forced_call: n / frames / seq / seq_proj / force_mel / mel_out / scores_out point to HOST arrays of n_sent entries."""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('n_sent', ctypes.c_int32), ('r', ctypes.c_int32), ('max_r', ctypes.c_int32),
                ('n', ctypes.POINTER(ctypes.c_int32)), ('frames', ctypes.POINTER(ctypes.c_int32)),
                ('seq', ctypes.POINTER(ctypes.c_void_p)), ('seq_proj', ctypes.POINTER(ctypes.c_void_p)),
                ('force_mel', ctypes.POINTER(ctypes.c_void_p)), ('mel_out', ctypes.POINTER(ctypes.c_void_p)),
                ('scores_out', ctypes.POINTER(ctypes.c_void_p)), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('stream', ctypes.c_void_p)]


class BigruCall(ctypes.Structure):
    """wrnn_bigru_call."""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('T', ctypes.c_int32), ('hidden', ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ('gi_fwd', 'gi_rev', 'w_hh_fwd', 'w_hh_rev', 'b_hh_fwd', 'b_hh_rev', 'out', 'stream')]


TACO_FRONT_MANY_MAX = 64     # WRNN_TACO_FRONT_MANY_MAX: sentences per wrnn_taco_encode_many / wrnn_taco_postnet_many / wrnn_bigru_many call


class BigruManyCall(ctypes.Structure):
    """wrnn_bigru_many_call: T points to a HOST array of n_seq lengths; gi_* / out hold the sequences one after another."""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('n_seq', ctypes.c_int32), ('hidden', ctypes.c_int32), ('T', ctypes.POINTER(ctypes.c_int32))] + \
               [(n, ctypes.c_void_p) for n in ('gi_fwd', 'gi_rev', 'w_hh_fwd', 'w_hh_rev', 'b_hh_fwd', 'b_hh_rev', 'out', 'stream')]


class CbhgWeights(ctypes.Structure):
    """wrnn_cbhg_weights: one CBHG's tensors (device pointers, the reference's state-dict layouts)."""
    _fields_ = [(n, ctypes.c_int32) for n in ('K', 'in_channels', 'proj1_channels', 'proj2_channels', 'channels', 'num_highways')] + \
               [(n, ctypes.c_void_p * 16) for n in ('bank_conv_w', 'bank_bn_w', 'bank_bn_b', 'bank_bn_mean', 'bank_bn_var')] + \
               [(n, ctypes.c_void_p) for n in ('proj1_conv_w', 'proj1_bn_w', 'proj1_bn_b', 'proj1_bn_mean', 'proj1_bn_var', 'proj2_conv_w',
                                               'proj2_bn_w', 'proj2_bn_b', 'proj2_bn_mean', 'proj2_bn_var', 'pre_highway_w')] + \
               [(n, ctypes.c_void_p * 4) for n in ('highway_w1', 'highway_b1', 'highway_w2', 'highway_b2')] + \
               [(n, ctypes.c_void_p) for n in ('rnn_w_ih', 'rnn_w_hh', 'rnn_b_ih', 'rnn_b_hh', 'rnn_w_ih_rev', 'rnn_w_hh_rev', 'rnn_b_ih_rev',
                                               'rnn_b_hh_rev')]


class TacoFrontWeights(ctypes.Structure):
    """wrnn_taco_front_weights (wrnn_taco_front_create)."""
    _fields_ = [('struct_bytes', ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ('n_symbols', 'embed_dims', 'prenet1', 'prenet2', 'encoder_proj_dims', 'n_mels', 'fft_bins')] + \
               [(n, ctypes.c_void_p) for n in ('embedding', 'prenet_fc1_w', 'prenet_fc1_b', 'prenet_fc2_w', 'prenet_fc2_b', 'encoder_proj_w',
                                               'post_proj_w')] + \
               [('encoder_cbhg', CbhgWeights), ('postnet', CbhgWeights)]


class Geometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('B', 'T', 'stride', 'L', 'hop', 'n_frames')]


class RunInfo(ctypes.Structure):
    _fields_ = [('kernel', ctypes.c_char_p)] + \
               [(n, ctypes.c_int32) for n in ('units_per_wg', 'clusters', 'depth', 'rounds', 'slab_steps', 'launches')]


class PlanTraits(ctypes.Structure):
    """wrnn_plan_traits (include/wavernn_amd.h): what the launch planner reads of a pack and its device (wrnn_debug_plan)."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_bytes', 'n_cus', 'mode', 'C', 'generic', 'gH', 'gF', 'gM', 'gA', 'sp_nbp', 'sp_max_blocks',
                                              'sp_fc')]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_bytes = ctypes.sizeof(PlanTraits)


class Options(ctypes.Structure):
    """wrnn_options (include/wavernn_amd.h): per-call options; nothing is read from the environment."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_bytes', 'algo', 'depth', 'clusters', 'cond_valu', 'slab_steps', 't_begin',
                                              't_end', 'tuning')] + \
               [('force_x', ctypes.c_void_p), ('logits', ctypes.c_void_p), ('phase_clocks', ctypes.c_void_p), ('timer', ctypes.c_void_p),
                ('info', ctypes.POINTER(RunInfo)), ('progress', ctypes.c_void_p), ('progress_user', ctypes.c_void_p),
                ('mel_stage', ctypes.c_int32), ('mel_rows', ctypes.c_int32), ('mel_scale', ctypes.c_int32),
                ('mel_taps', ctypes.c_void_p), ('seg_moff', ctypes.c_void_p), ('sparse_groups', ctypes.c_int32),
                ('noise_lib', ctypes.c_int32), ('noise_seed', ctypes.c_uint64), ('noise_seg_id', ctypes.c_void_p)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_bytes = ctypes.sizeof(Options)


class NllCall(ctypes.Structure):
    """wrnn_nll_call: the loss of a teacher-forced call (wrnn_nll: device pointers; wrnn_nll_host: host pointers)."""
    _fields_ = [('struct_bytes', ctypes.c_uint32), ('mode', ctypes.c_int32), ('n_classes', ctypes.c_int32), ('n_segments', ctypes.c_int32),
                ('T', ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ('logits', 'target', 'seg_len', 'nll', 'sum', 'stream')]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_bytes = ctypes.sizeof(NllCall)


class PostChunkCall(ctypes.Structure):
    """wrnn_post_chunk_call: the post-loop stage of a step range (wrnn_post_chunk: device pointers; wrnn_post_chunk_host: host pointers)."""
    _fields_ = [('struct_bytes', ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ('n_utt', 'T', 't0', 't1', 'n_classes', 'tail_len')] + \
               [(n, ctypes.c_void_p) for n in ('segments', 'row', 'wave_len', 'lut', 'tail', 'out64', 'out32', 'stream')]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_bytes = ctypes.sizeof(PostChunkCall)


#: wrnn_options.progress: void (*)(int32 steps_done, int32 T, int32 n_segments, void *user)
PROGRESS_FN = ctypes.CFUNCTYPE(None, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p)


class WrnnError(RuntimeError):
    pass


class ResidencyError(WrnnError):
    """WRNN_ERR_RESIDENCY on the FIRST slice of a step-sliced `auto` run: the persistent grid is not co-resident right now.  The
    callers that slice (WaveRNN.generate, generate_corpus) catch it and redo the call unsliced on the stream kernel."""


def build(verbose=False):
    """Compile the HIP sources for gfx950 into csrc/libwavernn_amd.so (hipcc cross-compiles without a GPU)."""
    cmd = [os.path.join(CSRC, 'build.sh')]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise WrnnError('building libwavernn_amd.so failed')
    global _lib
    _lib = None
    return SO_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Raises WrnnError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise WrnnError(f'{SO_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                        f'(or wavernn_amd/csrc/build.sh).  There is no CPU fallback.')
    # torch bundles its own libamdhip64; load it FIRST so this library binds to the same HIP runtime instance
    # (two HIP runtimes in one process do not see each other's devices / pointers).
    import torch  # noqa: F401
    L = ctypes.CDLL(SO_PATH)
    L.wrnn_last_error.restype = ctypes.c_char_p
    L.wrnn_abi_version.restype = ctypes.c_int
    L.wrnn_device_cus.argtypes = [ctypes.c_int]
    L.wrnn_pack_create.argtypes = [ctypes.POINTER(Weights), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.wrnn_pack_destroy.argtypes = [ctypes.c_void_p]
    L.wrnn_pack_destroy.restype = None
    L.wrnn_pack_weight_bytes.argtypes = [ctypes.c_void_p]
    L.wrnn_pack_weight_bytes.restype = ctypes.c_size_t
    L.wrnn_pack_sparse_blocks.argtypes = [ctypes.c_void_p]
    L.wrnn_pack_sparse_fc_blocks.argtypes = [ctypes.c_void_p]
    L.wrnn_pack_tile_sparse.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32 * 6), ctypes.POINTER(ctypes.c_int32 * 6)]
    L.wrnn_debug_tile_sparse_pack.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                              ctypes.POINTER(ctypes.c_int32)]
    L.wrnn_pack_tile_bf16.argtypes = [ctypes.c_void_p]
    L.wrnn_pack_tile_bf16.restype = ctypes.c_size_t
    L.wrnn_debug_tile_bf16_pack.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t]
    L.wrnn_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(Geometry), ctypes.POINTER(Options)]
    L.wrnn_workspace_bytes.restype = ctypes.c_size_t
    L.wrnn_generate.argtypes = [ctypes.c_void_p, ctypes.POINTER(Geometry), ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Options),
                                ctypes.c_void_p]
    L.wrnn_workspace_bytes_segments.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                ctypes.POINTER(Options)]
    L.wrnn_workspace_bytes_segments.restype = ctypes.c_size_t
    L.wrnn_generate_segments.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.POINTER(Options), ctypes.c_void_p]
    L.wrnn_generate_segments_watched.argtypes = L.wrnn_generate_segments.argtypes + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    L.wrnn_watch_words.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Options), ctypes.POINTER(ctypes.c_int32)]
    L.wrnn_debug_watch.argtypes = [ctypes.POINTER(PlanTraits), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Options), ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.wrnn_noise_fill.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.wrnn_noise_fill_host.argtypes = L.wrnn_noise_fill.argtypes[:8]
    L.wrnn_nll.argtypes = [ctypes.c_int, ctypes.POINTER(NllCall)]
    L.wrnn_nll_host.argtypes = [ctypes.POINTER(NllCall)]
    L.wrnn_plan_segments.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Options), ctypes.POINTER(RunInfo)]
    L.wrnn_timer_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.wrnn_timer_destroy.argtypes = [ctypes.c_void_p]
    L.wrnn_timer_destroy.restype = None
    L.wrnn_timer_ms.argtypes = [ctypes.c_void_p]
    L.wrnn_timer_ms.restype = ctypes.c_float
    L.wrnn_timer_launches.argtypes = [ctypes.c_void_p]
    L.wrnn_debug_read_exchange.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.POINTER(Options), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p]
    L.wrnn_debug_plan.argtypes = [ctypes.POINTER(PlanTraits), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Options),
                                  ctypes.POINTER(RunInfo), ctypes.POINTER(ctypes.c_size_t)]
    L.wrnn_pre_create.argtypes = [ctypes.POINTER(PreWeights), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.wrnn_pre_destroy.argtypes = [ctypes.c_void_p]
    L.wrnn_pre_destroy.restype = None
    L.wrnn_pre_hop.argtypes = [ctypes.c_void_p]
    L.wrnn_pre_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    L.wrnn_pre_workspace_bytes.restype = ctypes.c_size_t
    L.wrnn_pre_upsample.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.wrnn_pre_upsample_rows.argtypes = L.wrnn_pre_upsample.argtypes
    L.wrnn_pre_workspace_bytes_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(PreUtt), ctypes.c_int32, ctypes.c_int32]
    L.wrnn_pre_workspace_bytes_many.restype = ctypes.c_size_t
    L.wrnn_pre_upsample_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(PreUtt), ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.wrnn_pre_debug_host_handle.argtypes = [ctypes.POINTER(PreWeights), ctypes.POINTER(ctypes.c_void_p)]
    L.wrnn_pre_last_error.restype = ctypes.c_char_p
    L.wrnn_post_unfold.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                   ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.wrnn_post_last_error.restype = ctypes.c_char_p
    L.wrnn_post_chunk.argtypes = [ctypes.POINTER(PostChunkCall)]
    L.wrnn_post_chunk_host.argtypes = [ctypes.POINTER(PostChunkCall)]
    L.wrnn_taco_workspace_bytes.restype = ctypes.c_size_t
    L.wrnn_taco_decode.argtypes = [ctypes.c_int, ctypes.POINTER(TacoWeights), ctypes.POINTER(TacoCall)]
    L.wrnn_taco_status.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32 * 4), ctypes.c_void_p]
    L.wrnn_taco_last_error.restype = ctypes.c_char_p
    L.wrnn_taco_batch_workspace_bytes.argtypes = [ctypes.c_int32]
    L.wrnn_taco_batch_workspace_bytes.restype = ctypes.c_size_t
    L.wrnn_taco_decode_batch.argtypes = [ctypes.c_int, ctypes.POINTER(TacoWeights), ctypes.POINTER(TacoBatchCall)]
    L.wrnn_taco_forced_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    L.wrnn_taco_forced_workspace_bytes.restype = ctypes.c_size_t
    L.wrnn_taco_decode_forced.argtypes = [ctypes.c_int, ctypes.POINTER(TacoWeights), ctypes.POINTER(TacoForcedCall)]
    L.wrnn_taco_decode_batch_groups.argtypes = [ctypes.c_int, ctypes.POINTER(TacoWeights), ctypes.POINTER(ctypes.POINTER(TacoBatchCall)), ctypes.c_int32]
    L.wrnn_taco_decode_forced_groups.argtypes = [ctypes.c_int, ctypes.POINTER(TacoWeights), ctypes.POINTER(ctypes.POINTER(TacoForcedCall)), ctypes.c_int32]
    L.wrnn_debug_taco_group_of.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.wrnn_bigru.argtypes = [ctypes.c_int, ctypes.POINTER(BigruCall)]
    L.wrnn_taco_front_create.argtypes = [ctypes.POINTER(TacoFrontWeights), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.wrnn_taco_front_destroy.argtypes = [ctypes.c_void_p]
    L.wrnn_taco_front_destroy.restype = None
    L.wrnn_taco_front_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    L.wrnn_taco_front_workspace_bytes.restype = ctypes.c_size_t
    L.wrnn_taco_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.wrnn_taco_postnet.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_size_t, ctypes.c_void_p]
    L.wrnn_bigru_many.argtypes = [ctypes.c_int, ctypes.POINTER(BigruManyCall)]
    L.wrnn_taco_front_workspace_bytes_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    L.wrnn_taco_front_workspace_bytes_many.restype = ctypes.c_size_t
    L.wrnn_taco_encode_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.wrnn_taco_postnet_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.wrnn_taco_front_debug_host_handle.argtypes = [ctypes.POINTER(TacoFrontWeights), ctypes.POINTER(ctypes.c_void_p)]
    L.wrnn_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.wrnn_selftest.argtypes = [ctypes.c_int, ctypes.c_int]
    L.wrnn_selftest_metric.restype = ctypes.c_float
    _lib = L
    return L


def check(rc, what):
    if rc != WRNN_OK:
        raise WrnnError(f'{what} failed (rc={rc}): {lib().wrnn_last_error().decode()}')


def nll_host(mode, logits, target, seg_len=None, per_step=True):
    """`wrnn_nll_host`: the loss `wrnn_nll` computes on the device, by the calling thread.  logits (T, n, C) and target (n, T) float32 host arrays in
    the layouts of wrnn_options.logits / force_x, seg_len (n,) int32 or None.  Returns (nll (n, T) float32 or None, sum (n,) float64).  No HIP
    device is needed."""
    import numpy as np
    logits, target = np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(target, np.float32)
    T, n, C = logits.shape
    if target.shape != (n, T):
        raise ValueError(f'target has shape {target.shape}, the logits ask for {(n, T)}')
    lens = None if seg_len is None else np.ascontiguousarray(seg_len, np.int32)
    if lens is not None and lens.shape != (n,):
        raise ValueError('seg_len: one int32 per segment')
    nll, total = (np.empty((n, T), np.float32) if per_step else None), np.empty(n, np.float64)
    c = NllCall(mode=MODE_MOL if mode == 'MOL' else MODE_RAW, n_classes=C, n_segments=n, T=T, logits=logits.ctypes.data, target=target.ctypes.data,
                seg_len=None if lens is None else lens.ctypes.data, nll=None if nll is None else nll.ctypes.data, sum=total.ctypes.data)
    check(lib().wrnn_nll_host(ctypes.byref(c)), 'wrnn_nll_host')
    return nll, total


def post_chunk_host(segments, wave_len, t0, t1, tail, lut=None, row=None, want64=True, want32=False):
    """`wrnn_post_chunk_host`: steps [t0, t1) of the post-loop stage of unfolded utterances, by the calling thread.  segments (rows, T) float32,
    wave_len (n,) int32, tail (tail_len,) float64, lut (n_classes,) float64 or None, row (n,) int32 or None -- host arrays.  Returns
    (out64 (n, t1 - t0) float64 or None, out32 float32 or None).  No HIP device is needed."""
    import numpy as np
    segments = np.ascontiguousarray(segments, np.float32)
    wave_len, tail = np.ascontiguousarray(wave_len, np.int32), np.ascontiguousarray(tail, np.float64)
    lut = None if lut is None else np.ascontiguousarray(lut, np.float64)
    row = None if row is None else np.ascontiguousarray(row, np.int32)
    n = wave_len.shape[0]
    if segments.ndim != 2 or (row is not None and (row.shape != (n,) or (n and int(row.max()) >= segments.shape[0]))) or (row is None and n > segments.shape[0]):
        raise ValueError('segments: (rows, T); one row per utterance')
    w = max(0, int(t1) - int(t0))
    out64 = np.empty((n, w), np.float64) if want64 else None
    out32 = np.empty((n, w), np.float32) if want32 else None
    c = PostChunkCall(n_utt=n, T=segments.shape[1], t0=int(t0), t1=int(t1), n_classes=0 if lut is None else lut.shape[0], tail_len=tail.shape[0],
                      segments=segments.ctypes.data, row=None if row is None else row.ctypes.data, wave_len=wave_len.ctypes.data,
                      lut=None if lut is None else lut.ctypes.data, tail=tail.ctypes.data, out64=None if out64 is None else out64.ctypes.data,
                      out32=None if out32 is None else out32.ctypes.data)
    rc = lib().wrnn_post_chunk_host(ctypes.byref(c))
    if rc != WRNN_OK:
        raise WrnnError(f'wrnn_post_chunk_host failed (rc={rc}): {lib().wrnn_post_last_error().decode()}')
    return out64, out32


def noise_fill_host(mode, n_segments, n_classes, t_begin, t_end, seed, seg_id=None):
    """`wrnn_noise_fill_host`: the noise the library draws for steps [t_begin, t_end) (wrnn_options.noise_lib) as a host float32 array in the layout of
    `noise` -- MOL (t_end - t_begin, 11 * n_segments), RAW (t_end - t_begin, n_segments, n_classes).  No HIP device is needed."""
    import numpy as np
    mol = mode == 'MOL'
    out = np.empty((t_end - t_begin, 11 * n_segments) if mol else (t_end - t_begin, n_segments, n_classes), np.float32)
    ids = None if seg_id is None else np.ascontiguousarray(seg_id, dtype=np.uint64)
    if ids is not None and ids.shape != (n_segments,):
        raise ValueError('seg_id: one 64-bit id per segment')
    check(lib().wrnn_noise_fill_host(MODE_MOL if mol else MODE_RAW, n_segments, n_classes, t_begin, t_end, int(seed) & (2 ** 64 - 1),
                                     None if ids is None else ids.ctypes.data, out.ctypes.data), 'wrnn_noise_fill_host')
    return out


def tile_sparse_pack_host(W, gates):
    """`wrnn_debug_tile_sparse_pack`: the tile-sparse view (WRNN_ALGO_TILE_SPARSE) of one float32 matrix W (rows, K) of `gates` gates, as the library packs it.
    Returns dict(tab (rows / 16, 2), cols (groups, 4, 4) [kq][e], vals (groups, 64, 4) [lane][e], kept, total, admitted).  No HIP device is needed."""
    import numpy as np
    W = np.ascontiguousarray(W, np.float32)
    rows, K = W.shape
    tab = np.zeros((max(rows // 16, 1), 2), np.int32)
    kept, total, adm = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    groups = lib().wrnn_debug_tile_sparse_pack(W.ctypes.data, rows, K, gates, tab.ctypes.data, None, None, 0, ctypes.byref(kept), ctypes.byref(total), ctypes.byref(adm))
    if groups < 0:
        check(groups, 'wrnn_debug_tile_sparse_pack')
    cols, vals = np.full((groups, 4, 4), -1, np.int32), np.full((groups, 64, 4), np.nan, np.float32)
    check(min(0, lib().wrnn_debug_tile_sparse_pack(W.ctypes.data, rows, K, gates, tab.ctypes.data, cols.ctypes.data, vals.ctypes.data, groups,
                                                   ctypes.byref(kept), ctypes.byref(total), ctypes.byref(adm))), 'wrnn_debug_tile_sparse_pack')
    return dict(tab=tab, cols=cols, vals=vals, kept=int(kept.value), total=int(total.value), admitted=bool(adm.value))


def tile_bf16_pack_host(W):
    """`wrnn_debug_tile_bf16_pack`: the bf16 image (WRNN_ALGO_TILE_BF16) of one float32 matrix W (rows, K) as the library packs it: a uint16 array
    (ceil(K / 32) * rows + 64, 4, 8) -- [s * rows + row][kq][j] holds W[row][32 s + 4 j + kq] rounded to bfloat16 (round-to-nearest-even), k >= K and the
    last 64 rows +0.  Raises WrnnError when a value is not finite or rounds to +-inf.  No HIP device is needed."""
    import numpy as np
    W = np.ascontiguousarray(W, np.float32)
    rows, K = W.shape
    n = lib().wrnn_debug_tile_bf16_pack(W.ctypes.data, rows, K, None, 0)
    if n < 0:
        check(n, 'wrnn_debug_tile_bf16_pack')
    out = np.full(n, 0xFFFF, np.uint16)
    check(min(0, lib().wrnn_debug_tile_bf16_pack(W.ctypes.data, rows, K, out.ctypes.data, n)), 'wrnn_debug_tile_bf16_pack')
    return out.reshape(-1, 4, 8)


def watch_words_host(traits, n_segments, T, opts=None, progress=None, progress_words=0, progress_every=1):
    """`wrnn_debug_watch`: what a watched call (`wrnn_generate_segments_watched`) answers for a pack with these `PlanTraits` -- the words it writes, or
    WrnnError with the library's refusal.  progress=None: as `wrnn_watch_words` (kernel and step range only); True / False: a non-NULL / NULL `progress`
    of `progress_words` words, published every `progress_every` steps.  No HIP device is needed."""
    words = ctypes.c_int32(-1)
    check(lib().wrnn_debug_watch(ctypes.byref(traits), int(n_segments), int(T), None if opts is None else ctypes.byref(opts),
                                 -1 if progress is None else int(bool(progress)), int(progress_words), int(progress_every), ctypes.byref(words)), 'wrnn_debug_watch')
    return int(words.value)

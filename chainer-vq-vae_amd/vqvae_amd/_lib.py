"""ctypes binding of libvqvae_hip.so: one HEADERS entry per header under include/.

An entry holds the header's file name, the words its version error uses, the version this package binds and the
prototype table; load() binds every table, then compares every version.  A Structure names the C typedef it mirrors
in _c_name_.  An upper-case integer N of this module mirrors the macro VQVAE_N of the header whose stem is the
longest prefix of N (KMEANS_BLOCK: vqvae_kmeans.h), or of vqvae_hip.h when no stem is one (EW_ADD, GEN_MAX_N);
UNMIRRORED lists the few that mirror nothing public.  tests/test_host_abi.py holds all of this against the headers.

There is no CPU fallback: if the shared library is missing, importing anything
that needs it raises, and every compute entry point requires a gfx950 device.
"""
import collections
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), 'libvqvae_hip.so')

c_void_p, c_int, c_long, c_size_t = C.c_void_p, C.c_int, C.c_long, C.c_size_t
c_float, c_double, c_char_p = C.c_float, C.c_double, C.c_char_p
P = c_void_p                      # every device pointer crosses as an integer address
PP = C.POINTER(c_void_p)          # host array of device pointers


def ptr_array(arrays):
    """Host array of device pointers (None -> NULL) for the resstack entry points."""
    return (c_void_p * len(arrays))(*[None if a is None else a.ptr for a in arrays])


class Conv1dDesc(C.Structure):
    _c_name_ = 'vqvae_conv1d_desc'
    _fields_ = [(n, c_int) for n in
                ('B', 'Cin', 'Tin', 'Cout', 'Tout', 'K', 'stride', 'pad', 'dil', 'relu')]


class ResblockDesc(C.Structure):
    _c_name_ = 'vqvae_resblock_desc'
    _fields_ = [(n, c_int) for n in ('B', 'T', 'Cr', 'Cd', 'Cs', 'Cc', 'K', 'dil', 'storage')]


class ResblockParams(C.Structure):
    _c_name_ = 'vqvae_resblock_params'
    _fields_ = [(n, P) for n in ('Wd', 'bd', 'Wc', 'bc', 'Wr', 'br', 'Ws', 'bs')]


class ResblockCproj(C.Structure):
    _c_name_ = 'vqvae_resblock_cproj'
    _fields_ = [('P', P), ('P_bstride', c_long), ('Tl', c_int), ('v0', P), ('w0', P), ('w1', P), ('P_has_bd', c_int), ('P_amax', P)]


class ResblockAmax(C.Structure):
    """Device uint32 slots (float bit patterns of absolute maxima), matmul mode 3."""
    _c_name_ = 'vqvae_resblock_amax'
    _fields_ = [(n, P) for n in ('x', 'res', 'g_res', 'g_skip', 'gh', 'gx', 'x_max', 'res_scale', 'gh_scale',
                                 'pb_part', 'pb_v0', 'pb_w0', 'pb_w1')] + [('pb_Tl', c_int)]


class Conv1dAmax(C.Structure):
    _c_name_ = 'vqvae_conv1d_amax'
    _fields_ = [(n, P) for n in ('x', 'gy', 'out', 'packed')]


class ResblockGrads(C.Structure):
    _c_name_ = 'vqvae_resblock_grads'
    _fields_ = [(n, P) for n in ('gWd', 'gbd', 'gWc', 'gbc', 'gWr', 'gbr', 'gWs', 'gbs')]


class GenBlock(C.Structure):
    _c_name_ = 'vqvae_gen_block'
    _fields_ = [(n, P) for n in ('conv_W', 'conv_b', 'cond_W', 'cond_b', 'res_W', 'res_b',
                                 'skip_W', 'skip_b', 'ring')] + [('dilation', c_int)]


class GenDesc(C.Structure):
    _c_name_ = 'vqvae_gen_desc'
    _fields_ = ([(n, c_int) for n in ('n', 'n_blocks', 'input_dim', 'residual', 'dilated', 'skip',
                                      'cond_dim', 'out_dim', 'sample_mode')]
                + [('log_scale_min', c_float)]
                + [(n, P) for n in ('embed_W', 'embed_b', 'proj1_W', 'proj1_b', 'proj2_W', 'proj2_b')]
                + [('blocks', C.POINTER(GenBlock))]
                + [(n, P) for n in ('step', 'x_cur', 'x_prev', 'h0', 'h1', 'z', 'skip_acc', 's1',
                                    'logits', 'cond')]
                + [('cond_bstride', c_long), ('cond_cstride', c_long), ('cond_follows_step', c_int),
                   ('uniforms', P), ('n_uniform', c_int), ('forced_next', P), ('out', P),
                   ('out_bstride', c_long), ('logits_out', P), ('max_steps', c_int)])


class GenSampling(C.Structure):
    """Device arrays of n entries, NULL = neutral for every sequence."""
    _c_name_ = 'vqvae_gen_sampling'
    _fields_ = [(n, P) for n in ('temperature', 'top_k', 'top_p')]


class GenSlots(C.Structure):
    """The slot table of lockstep generation with refill."""
    _c_name_ = 'vqvae_gen_slots'
    _fields_ = [('n_seq', c_int), ('steps', P), ('queue', P), ('n_queue', c_int), ('next', P), ('slot_seq', P),
                ('slot_t', P), ('live', P), ('started', P)]


class GenLatentCond(C.Structure):
    """The latent-rate condition of lockstep generation."""
    _c_name_ = 'vqvae_gen_latent_cond'
    _fields_ = [('local', P), ('local_off', P), ('tl', P), ('global_vec', P), ('col_seq', P), ('column', P),
                ('n_seq', c_int), ('Cl', c_int), ('G', c_int), ('upscale', c_int)]


class GenRng(C.Structure):
    """The seed and the device array of stream ids (NULL = the identity)."""
    _c_name_ = 'vqvae_gen_rng'
    _fields_ = [('seed', C.c_uint64), ('ids', P)]


class Corpus(C.Structure):
    """The device-resident corpus, or a view of it (view NULL = the identity)."""
    _c_name_ = 'vqvae_corpus'
    _fields_ = [(n, P) for n in ('samples', 'offset', 'length', 'speaker', 'view')] + [('n_view', C.c_int32)]


class RaggedConvDesc(C.Structure):
    """One conv stage over a ragged batch."""
    _c_name_ = 'vqvae_ragged_conv_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'cin', 'cout', 'K', 'stride', 'pad', 'dil', 'relu', 'blocked_out')] + \
               [('ttot_out', C.c_int64), ('x_cstride', C.c_int64)]


class MetricsDesc(C.Structure):
    """One STFT / log-mel / distance call over a ragged list."""
    _c_name_ = 'vqvae_metrics_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'n_fft', 'hop', 'n_mels', 'n_mcep')] + [('floor', c_float), ('ftot', C.c_int64), ('stride', C.c_int64)]


class PitchDesc(C.Structure):
    """One YIN / pair-statistics call over a ragged list."""
    _c_name_ = 'vqvae_pitch_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'sr', 'frame', 'hop')] + \
               [(n, C.c_double) for n in ('fmin', 'fmax', 'threshold', 'min_power')] + [('ftot', C.c_int64)]


class RdecDesc(C.Structure):
    """One chunk of the ragged decoder pass."""
    _c_name_ = 'vqvae_rdec_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'R', 'D', 'S', 'Q', 'Cl', 'G', 'n_blocks', 'upscale', 'reserved')] + \
               [('ttot', C.c_int64), ('tltot', C.c_int64)]


class RdecTables(C.Structure):
    """The device tables of one chunk of the ragged decoder pass."""
    _c_name_ = 'vqvae_rdec_tables'
    _fields_ = [(n, P) for n in ('off', 'qoff', 'latoff', 'tl')]


class AlignDesc(C.Structure):
    """One chunk of pairs to align."""
    _c_name_ = 'vqvae_align_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'n_mels', 'n_mcep', 'max_short')] + \
               [(n, C.c_int64) for n in ('fa_tot', 'fb_tot', 'stride_a', 'stride_b', 'cells', 'ptot')]


class AlignTables(C.Structure):
    """The device tables of one chunk of pairs to align."""
    _c_name_ = 'vqvae_align_tables'
    _fields_ = [(n, P) for n in ('off_a', 'off_b', 'cell_off', 'path_off')]


class CodesRunsDesc(C.Structure):
    _c_name_ = 'vqvae_codes_runs_desc'
    _fields_ = [('n', C.c_int32), ('max_run', C.c_int32), ('total', C.c_int64)]


class CodesHistDesc(C.Structure):
    _c_name_ = 'vqvae_codes_hist_desc'
    _fields_ = [(n, C.c_int32) for n in ('n', 'k', 'groups', 'bigrams', 'accumulate', 'reserved')] + [('total', C.c_int64)]


class CodesPairDesc(C.Structure):
    _c_name_ = 'vqvae_codes_pair_desc'
    _fields_ = [('n', C.c_int32), ('max_short', C.c_int32), ('total_a', C.c_int64), ('total_b', C.c_int64)]


class CodesPairTables(C.Structure):
    """The device tables of the two sides of a list of code-string pairs."""
    _c_name_ = 'vqvae_codes_pair_tables'
    _fields_ = [(n, P) for n in ('start_a', 'len_a', 'start_b', 'len_b')]


class Header(collections.namedtuple('Header', 'file words version prototypes')):
    """One header of include/: what the version error calls it, the version bound, name -> (restype, argtypes)."""

    @property
    def version_symbol(self):
        stem = self.file[len('vqvae_'):-len('.h')]
        return 'vqvae_abi_version' if stem == 'hip' else 'vqvae_%s_abi_version' % stem


HEADERS = {}                      # file name -> Header, in load order


def _header(file, words, version, prototypes):
    HEADERS[file] = Header(file, words, version, prototypes)


# each table IS the list of symbols its header declares
_header('vqvae_hip.h', 'ABI', 5, {
    'vqvae_last_error_string': (c_char_p, []),
    'vqvae_abi_version': (c_int, []),
    'vqvae_device_count': (c_int, [C.POINTER(c_int)]),
    'vqvae_set_device': (c_int, [c_int]),
    'vqvae_device_info': (c_int, [c_char_p, c_int, C.POINTER(c_int), C.POINTER(c_size_t)]),
    'vqvae_device_pci_bus_id': (c_int, [c_char_p, c_int]),
    'vqvae_malloc': (c_int, [C.POINTER(c_void_p), c_size_t]),
    'vqvae_free': (c_int, [P]),
    'vqvae_memcpy_h2d': (c_int, [P, c_void_p, c_size_t, P]),
    'vqvae_memcpy_d2h': (c_int, [c_void_p, P, c_size_t, P]),
    'vqvae_host_alloc': (c_int, [C.POINTER(c_void_p), c_size_t]),
    'vqvae_host_free': (c_int, [c_void_p]),
    'vqvae_memcpy_h2d_async': (c_int, [P, c_void_p, c_size_t, P]),
    'vqvae_memcpy_d2d': (c_int, [P, P, c_size_t, P]),
    'vqvae_memcpy2d_d2d': (c_int, [P, c_size_t, P, c_size_t, c_size_t, c_size_t, P]),
    'vqvae_memset': (c_int, [P, c_int, c_size_t, P]),
    'vqvae_stream_create': (c_int, [C.POINTER(c_void_p)]),
    'vqvae_stream_destroy': (c_int, [P]),
    'vqvae_stream_synchronize': (c_int, [P]),
    'vqvae_device_synchronize': (c_int, []),
    'vqvae_event_create': (c_int, [C.POINTER(c_void_p)]),
    'vqvae_event_destroy': (c_int, [P]),
    'vqvae_event_record': (c_int, [P, P]),
    'vqvae_event_synchronize': (c_int, [P]),
    'vqvae_stream_wait_event': (c_int, [P, P]),
    'vqvae_event_elapsed_ms': (c_int, [C.POINTER(c_float), P, P]),
    'vqvae_prof_enable': (c_int, [c_int]),
    'vqvae_prof_reset': (c_int, []),
    'vqvae_prof_read': (c_int, [c_int, C.POINTER(c_double), C.POINTER(c_int)]),
    'vqvae_set_matmul_dtype': (c_int, [c_int]),
    'vqvae_get_matmul_dtype': (c_int, []),
    'vqvae_set_wgrad_impl': (c_int, [c_int]),
    'vqvae_absmax': (c_int, [P, c_size_t, P, P]),
    'vqvae_set_f32x2_min_gflop': (c_int, [c_double]),
    'vqvae_conv1d_workspace_bytes': (c_size_t, [C.POINTER(Conv1dDesc)]),
    'vqvae_conv1d_fwd': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, P, c_size_t, P]),
    'vqvae_conv1d_bwd_data': (c_int, [C.POINTER(Conv1dDesc), P, P, P, c_int, P, c_size_t, P]),
    'vqvae_conv1d_bwd_weight': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, c_int, P, c_size_t, P]),
    'vqvae_conv1d_uses_f32x2': (c_int, [C.POINTER(Conv1dDesc)]),
    'vqvae_conv1d_forms': (c_int, [C.POINTER(Conv1dDesc), c_int]),
    'vqvae_conv1d_packed_bytes': (c_size_t, [C.POINTER(Conv1dDesc), c_int]),
    'vqvae_conv1d_pack': (c_int, [c_int, C.POINTER(Conv1dDesc), C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_void_p), P]),
    'vqvae_conv1d_fwd_amax': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, P, c_size_t, C.POINTER(Conv1dAmax), P]),
    'vqvae_conv1d_bwd_data_amax': (c_int, [C.POINTER(Conv1dDesc), P, P, P, c_int, P, c_size_t, C.POINTER(Conv1dAmax), P]),
    'vqvae_conv1d_bwd_weight_amax': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, c_int, P, c_size_t,
                                             C.POINTER(Conv1dAmax), P]),
    'vqvae_resblock_workspace_bytes': (c_size_t, [C.POINTER(ResblockDesc)]),
    'vqvae_resblock_fwd': (c_int, [C.POINTER(ResblockDesc), C.POINTER(ResblockParams), P, P,
                                   C.POINTER(ResblockCproj), P, P, c_int, P, P, P, c_size_t, P]),
    'vqvae_resblock_bwd': (c_int, [C.POINTER(ResblockDesc), C.POINTER(ResblockParams), P, P, P, P,
                                   P, P, P, P, c_int, P, C.POINTER(ResblockGrads), c_int, P,
                                   c_size_t, P]),
    'vqvae_resblock_wgrad': (c_int, [C.POINTER(ResblockDesc), P, P, P, P, c_int, P, c_size_t, P]),
    'vqvae_resstack_packed_bytes': (c_size_t, [C.POINTER(ResblockDesc)]),
    'vqvae_resstack_pack': (c_int, [C.POINTER(ResblockDesc), c_int, C.POINTER(ResblockParams),
                                    C.POINTER(c_int), P, c_size_t, P]),
    'vqvae_resblock_fwd_packed': (c_int, [C.POINTER(ResblockDesc), C.POINTER(ResblockParams), P,
                                          C.POINTER(ResblockCproj), P, P, P, P, c_size_t, P,
                                          C.POINTER(ResblockAmax), P]),
    'vqvae_resblock_bwd_packed': (c_int, [C.POINTER(ResblockDesc), C.POINTER(ResblockParams), P, P, P,
                                          P, P, P, P, P, c_size_t, P, C.POINTER(ResblockAmax), P]),
    'vqvae_resstack_workspace_bytes': (c_size_t, [C.POINTER(ResblockDesc), c_int]),
    'vqvae_resstack_skip_fwd': (c_int, [C.POINTER(ResblockDesc), c_int, PP, PP, PP, P, c_int, c_int, P,
                                        c_size_t, P, P]),
    'vqvae_resstack_skip_prepare': (c_int, [C.POINTER(ResblockDesc), c_int, PP, PP, P, c_size_t, P]),
    'vqvae_resstack_skip_fwd_prepared': (c_int, [C.POINTER(ResblockDesc), c_int, PP, P, c_int, c_int, P, c_size_t, P, P]),
    'vqvae_conv1d_bwd_data_relu': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, P, c_size_t, C.POINTER(Conv1dAmax), P]),
    'vqvae_resstack_gcond_bwd': (c_int, [C.POINTER(ResblockDesc), c_int, PP, PP, P, c_int, P,
                                         c_size_t, P]),
    'vqvae_resstack_skip_wgrad': (c_int, [C.POINTER(ResblockDesc), c_int, P, PP, PP, PP, c_int, P,
                                          c_size_t, P, P]),
    'vqvae_resstack_res_wgrad': (c_int, [C.POINTER(ResblockDesc), c_int, PP, PP, PP, PP, c_int, P,
                                         c_size_t, PP, P]),
    'vqvae_resstack_dil_wgrad_workspace_bytes': (c_size_t, [C.POINTER(ResblockDesc), c_int]),
    'vqvae_resstack_dil_wgrad': (c_int, [C.POINTER(ResblockDesc), c_int, C.POINTER(c_int), PP, PP, PP, PP,
                                         c_int, P, c_size_t, PP, PP, P]),
    'vqvae_vq_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'vqvae_vq_nearest_fwd': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P,
                                     c_size_t, P]),
    'vqvae_vq_grad_w': (c_int, [P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_size_t, P]),
    'vqvae_vq_paths': (c_int, [c_int, c_int, c_int, c_int, c_int]),
    'vqvae_upsample_linear_fwd': (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, P, P, c_long, P]),
    'vqvae_upsample_linear_bwd': (c_int, [P, c_long, c_int, c_int, c_int, c_int, P, P, P, P, P, P,
                                          P, c_long, P]),
    'vqvae_upsample_linear_bwd_blocks': (c_int, [P, c_int, c_long, c_long, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, c_long, c_long, P]),
    'vqvae_upsample_linear_bwd_bf16': (c_int, [P, c_long, c_int, c_int, c_int, c_int, P, P, P, P, P, P,
                                               P, c_long, P]),
    'vqvae_resblock_bf16_storage': (c_int, [C.POINTER(ResblockDesc)]),
    'vqvae_resblock_f16x2_storage': (c_int, [C.POINTER(ResblockDesc)]),
    'vqvae_set_presplit': (c_int, [c_int]),
    'vqvae_get_fused_pullback': (c_int, [C.POINTER(ResblockDesc)]),
    'vqvae_pullback_reduce': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    'vqvae_pullback_reduce_into': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    'vqvae_f32x2_contract_check': (c_int, [c_int, PP, PP, c_int, P, P]),
    'vqvae_convstack_supported': (c_int, [c_int, c_int, c_int, C.POINTER(c_int)]),
    'vqvae_convstack_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'vqvae_convstack_fwd': (c_int, [c_int, c_int, c_int, c_int, C.POINTER(c_int), P, PP, PP, PP, P]),
    'vqvae_convstack_bwd': (c_int, [c_int, c_int, c_int, c_int, C.POINTER(c_int), P, PP, PP, P, P, PP, PP, c_int, P, c_size_t, P]),
    'vqvae_conv_s2_bwd_supported': (c_int, [c_int] * 8),
    'vqvae_conv_s2_bwd_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'vqvae_conv_s2_bwd': (c_int, [c_int, c_int, c_int, c_int, P, P, P, c_int, P, P, P, c_int, P, c_size_t, P]),
    'vqvae_upsample_linear_bwd_f16x2': (c_int, [P, c_long, c_int, c_int, c_int, c_int, P, P, P, P, P, P,
                                                P, c_long, P, P]),
    'vqvae_mulaw_bins': (c_int, [P, c_size_t, P, c_int, P, P]),
    'vqvae_onehot': (c_int, [P, c_long, c_int, c_int, c_int, P, P]),
    'vqvae_embed_gather_fwd': (c_int, [P, c_long, c_int, c_int, P, P, c_int, c_int, c_int, P, P]),
    'vqvae_embed_gather_bound': (c_int, [P, P, c_int, c_int, c_int, P, P]),
    'vqvae_embed_onehot_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'vqvae_embed_onehot_fwd': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, c_size_t, P]),
    'vqvae_embed_onehot_wgrad': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P,
                                         c_size_t, P]),
    'vqvae_conv1d_fwd_cond': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, P, c_size_t, P, P]),
    'vqvae_conv1d_bwd_weight_cond': (c_int, [C.POINTER(Conv1dDesc), P, P, P, P, c_int, P, c_size_t, P, P]),
    'vqvae_concat': (c_int, [P, PP, c_int, c_size_t, P]),
    'vqvae_split': (c_int, [P, PP, c_int, c_size_t, c_int, P]),
    'vqvae_copy_list': (c_int, [c_int, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(c_size_t), P]),
    'vqvae_embed_broadcast_fwd': (c_int, [P, P, c_int, c_int, c_int, P, c_long, P]),
    'vqvae_embed_broadcast_bwd': (c_int, [P, c_long, P, c_int, c_int, c_int, c_int, P, c_int, P,
                                          c_size_t, P]),
    'vqvae_softmax_xent_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'vqvae_softmax_xent_fwd': (c_int, [P, P, c_int, c_int, c_int, P, P, P, c_size_t, P]),
    'vqvae_softmax_xent_bwd': (c_int, [P, P, P, P, c_int, c_int, c_int, P, P]),
    'vqvae_softmax_xent_bwd_amax': (c_int, [P, P, P, P, c_int, c_int, c_int, P, P, P]),
    'vqvae_mol_nll_fwd': (c_int, [P, P, c_int, c_int, c_int, c_int, c_float, P, P, c_size_t, P]),
    'vqvae_mol_nll_bwd': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_float, P, P]),
    'vqvae_elementwise': (c_int, [c_int, c_size_t, P, P, P, c_float, c_float, P]),
    'vqvae_sum': (c_int, [P, c_size_t, c_float, P, P, c_size_t, P]),
    'vqvae_sqdiff_mean': (c_int, [P, P, c_size_t, P, P, c_size_t, P]),
    'vqvae_sqdiff_mean_bwd': (c_int, [P, P, P, c_size_t, P, P, P]),
    'vqvae_adam_step': (c_int, [P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, P]),
    'vqvae_adam_step_dev': (c_int, [P, P, P, P, c_size_t, P, P, c_double, c_double, c_double, P]),
    'vqvae_ema_step': (c_int, [P, P, c_size_t, c_double, P]),
    'vqvae_comm_unique_id': (c_int, [c_char_p]),
    'vqvae_comm_init': (c_int, [C.POINTER(c_void_p), c_int, c_int, c_char_p]),
    'vqvae_comm_allreduce_sum_f32': (c_int, [P, P, c_size_t, P]),
    'vqvae_comm_allreduce_max_f32': (c_int, [P, P, c_size_t, P]),
    'vqvae_comm_count': (c_int, [P, C.POINTER(c_int)]),
    'vqvae_comm_destroy': (c_int, [P]),
    'vqvae_wavenet_gen_step': (c_int, [C.POINTER(GenDesc), P]),
    'vqvae_wavenet_gen_run_workspace_bytes': (c_size_t, [C.POINTER(GenDesc)]),
    'vqvae_wavenet_gen_run': (c_int, [C.POINTER(GenDesc), c_int, c_int, P, c_size_t, P]),
    'vqvae_wavenet_gen_run_concurrency': (c_int, [C.POINTER(GenDesc)]),
    'vqvae_graph_capture_begin': (c_int, [P]),
    'vqvae_graph_capture_begin_relaxed': (c_int, [P]),
    'vqvae_graph_capture_end': (c_int, [P, C.POINTER(c_void_p)]),
    'vqvae_graph_launch': (c_int, [P, P]),
    'vqvae_graph_destroy': (c_int, [P]),
})

# include/vqvae_codebook.h: codebook statistics and re-seeding
_header('vqvae_codebook.h', 'codebook ABI', 1, {
    'vqvae_codebook_abi_version': (c_int, []),
    'vqvae_codebook_observe': (c_int, [P, P, c_int, c_int, c_int, c_int, c_float, C.c_uint64, P, P, P, P, P, P]),
    'vqvae_codebook_reseed': (c_int, [P, P, P, c_int, c_int, P, P, c_float, c_float, P, P, P]),
})
CODEBOOK_STATS_WORDS = 8
CODEBOOK_LDS_MAX_K = 16384

# include/vqvae_vq_ema.h: EMA codebook updates
_header('vqvae_vq_ema.h', 'EMA-codebook ABI', 1, {
    'vqvae_vq_ema_abi_version': (c_int, []),
    'vqvae_vq_ema_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'vqvae_vq_ema_accumulate': (c_int, [P, P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    'vqvae_vq_ema_apply': (c_int, [P, P, P, P, c_int, c_int, c_float, c_float, P]),
    'vqvae_vq_ema_reset': (c_int, [P, P, P, c_int, c_int, P, P]),
})
VQ_EMA_PIECE = 512
VQ_EMA_SMALL_MAX_N = 4096
VQ_EMA_MAX_N = 1 << 24

# include/vqvae_kmeans.h: k-means initialisation of the codebook
_header('vqvae_kmeans.h', 'k-means ABI', 1, {
    'vqvae_kmeans_abi_version': (c_int, []),
    'vqvae_kmeans_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'vqvae_kmeans_collect': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, P]),
    'vqvae_kmeans_seed': (c_int, [P, c_int, c_int, c_int, C.c_uint64, P, P, P, P, c_size_t, P]),
    'vqvae_kmeans_update': (c_int, [P, c_int, c_int, c_int, P, C.c_uint64, c_int, P, P, P]),
    'vqvae_kmeans_inertia': (c_int, [P, P, P, c_int, c_int, c_int, P, P, c_size_t, P]),
})
KMEANS_BLOCK = 256
KMEANS_MAX_N = 1 << 24
KMEANS_MAX_D = 4096

# include/vqvae_optim.h: optimizer hooks (gradient norms, clipping, the non-finite guard)
_header('vqvae_optim.h', 'optimizer-hook ABI', 1, {
    'vqvae_optim_abi_version': (c_int, []),
    'vqvae_optim_plan_items': (c_int, [C.POINTER(C.c_int64), c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'vqvae_optim_workspace_bytes': (c_size_t, [c_int]),
    'vqvae_optim_state_bytes': (c_size_t, [c_int, c_int, c_int]),
    'vqvae_optim_sumsq': (c_int, [P, c_size_t, P, c_int, P, c_int, P, P, c_int, c_int, c_double, c_int, P, P, c_size_t, P]),
    'vqvae_optim_adam_step_hooked': (c_int, [P, P, P, P, c_size_t, c_double, P, P, c_double, c_double, c_double, P,
                                             c_int, P]),
})
OPTIM_CHUNK = 4096
OPTIM_THREADS = 256
OPTIM_STATE_HEADER = 64
OPTIM_GUARD = 1

# include/vqvae_sampling.h: sampling controls for generation (temperature, top-k, top-p, greedy)
_header('vqvae_sampling.h', 'sampling ABI', 1, {
    'vqvae_sampling_abi_version': (c_int, []),
    'vqvae_wavenet_gen_step_sampled': (c_int, [C.POINTER(GenDesc), C.POINTER(GenSampling), P]),
    'vqvae_sample_logits': (c_int, [P, c_int, c_int, c_int, c_float, P, c_int, C.POINTER(GenSampling), P, P, P]),
})
SAMPLING_MAX_CLASSES = 1024

# include/vqvae_gen_slots.h: lockstep generation with refill (slots, queue and scheduler on the device)
_header('vqvae_gen_slots.h', 'slot-generation ABI', 1, {
    'vqvae_gen_slots_abi_version': (c_int, []),
    'vqvae_gen_slots_init': (c_int, [C.POINTER(GenDesc), C.POINTER(GenSlots), P]),
    'vqvae_wavenet_gen_step_slots': (c_int, [C.POINTER(GenDesc), C.POINTER(GenSlots), C.POINTER(GenSampling), P]),
})

# include/vqvae_gen_cond.h: the condition column of a lockstep step from the latent-rate condition
_header('vqvae_gen_cond.h', 'latent-condition ABI', 1, {
    'vqvae_gen_cond_abi_version': (c_int, []),
    'vqvae_gen_cond_column': (c_int, [C.POINTER(GenLatentCond), C.POINTER(GenDesc), C.POINTER(GenSlots), P]),
})

# include/vqvae_gen_rng.h: the uniforms of generation drawn on the device (Philox4x32-10)
_header('vqvae_gen_rng.h', 'device-uniforms ABI', 1, {
    'vqvae_gen_rng_abi_version': (c_int, []),
    'vqvae_gen_rng_fill': (c_int, [C.POINTER(GenRng), c_int, c_int, c_int, c_int, P, P]),
    'vqvae_sample_logits_rng': (c_int, [P, c_int, c_int, c_int, c_float, C.POINTER(GenRng), c_int, c_int,
                                        C.POINTER(GenSampling), P, P, P]),
    'vqvae_wavenet_gen_step_rng': (c_int, [C.POINTER(GenDesc), C.POINTER(GenSampling), C.POINTER(GenRng), P]),
    'vqvae_wavenet_gen_step_slots_rng': (c_int, [C.POINTER(GenDesc), C.POINTER(GenSlots), C.POINTER(GenSampling),
                                                 C.POINTER(GenRng), P]),
})

# include/vqvae_corpus.h: minibatches drawn on the device from a corpus that lives there
_header('vqvae_corpus.h', 'resident-corpus ABI', 1, {
    'vqvae_corpus_abi_version': (c_int, []),
    'vqvae_corpus_draw': (c_int, [C.POINTER(Corpus), C.c_uint64, c_int, C.c_uint64, c_int, c_int, c_int, c_int, c_int, P, c_int,
                                  P, P, P, P, P, P, P]),
})

# include/vqvae_ingest.h: decode, resample, trim and normalise raw audio into a corpus's waveforms
_header('vqvae_ingest.h', 'ingest ABI', 1, {
    'vqvae_ingest_abi_version': (c_int, []),
    'vqvae_ingest_workspace_bytes': (c_size_t, [c_int, c_int]),
    'vqvae_ingest_resample': (c_int, [P, c_int, c_int, P, P, c_int, c_int, P, c_int, c_int, c_int, P, P, c_int, P]),
    'vqvae_ingest_trim_bounds': (c_int, [P, P, P, c_int, c_int, c_double, P, c_size_t, P, P]),
    'vqvae_ingest_pack': (c_int, [P, P, P, P, c_int, c_int, P, P]),
})
INGEST_TILE = 1024
INGEST_MAX_TAPS = 1 << 22
INGEST_MAX_WINDOW = 16384

# include/vqvae_ragged.h: the encoder's and ConditionEmbed's convs over a ragged batch and the two gathers
_header('vqvae_ragged.h', 'ragged-front-end ABI', 1, {
    'vqvae_ragged_abi_version': (c_int, []),
    'vqvae_ragged_conv_workspace_bytes': (c_size_t, [C.POINTER(RaggedConvDesc)]),
    'vqvae_ragged_conv_fwd': (c_int, [C.POINTER(RaggedConvDesc), P, P, P, P, P, P, P, P, c_size_t, P]),
    'vqvae_ragged_code_gather': (c_int, [P, P, C.c_int64, c_int, c_int, P, P]),
    'vqvae_ragged_speaker_gather': (c_int, [P, P, c_int, c_int, c_int, P, P]),
})

# include/vqvae_metrics.h: ragged STFT, log-mel and the per-utterance distances
_header('vqvae_metrics.h', 'audio-metrics ABI', 1, {
    'vqvae_metrics_abi_version': (c_int, []),
    'vqvae_metrics_stft_mel_workspace_bytes': (c_size_t, [C.POINTER(MetricsDesc)]),
    'vqvae_metrics_distances_workspace_bytes': (c_size_t, [C.POINTER(MetricsDesc)]),
    'vqvae_metrics_stft_mel': (c_int, [C.POINTER(MetricsDesc), P, P, P, P, P, P, P, P, P, c_size_t, P]),
    'vqvae_metrics_distances': (c_int, [C.POINTER(MetricsDesc), P, P, P, P, P, P, P, P, c_size_t, P]),
})
METRICS_TILE = 32
METRICS_THREADS = 256
METRICS_MAX_NFFT = 2048
METRICS_MAX_MELS = 128

# include/vqvae_pitch.h: ragged YIN F0 and the per-pair pitch statistics
_header('vqvae_pitch.h', 'pitch ABI', 1, {
    'vqvae_pitch_abi_version': (c_int, []),
    'vqvae_pitch_yin_workspace_bytes': (c_size_t, [C.POINTER(PitchDesc)]),
    'vqvae_pitch_compare_workspace_bytes': (c_size_t, [C.POINTER(PitchDesc)]),
    'vqvae_pitch_yin': (c_int, [C.POINTER(PitchDesc), P, P, P, P, P, P, c_size_t, P]),
    'vqvae_pitch_compare': (c_int, [C.POINTER(PitchDesc), P, P, P, P, P, c_size_t, P]),
})
PITCH_THREADS = 256
PITCH_MAX_TILE = 4
PITCH_MAX_FRAME = 2048
PITCH_COLUMNS = 8

# include/vqvae_ragged_decoder.h: the teacher-forced decoder pass over a ragged list (held-out likelihood)
_header('vqvae_ragged_decoder.h', 'ragged-decoder ABI', 1, {
    'vqvae_ragged_decoder_abi_version': (c_int, []),
    'vqvae_rdec_workspace_bytes': (c_size_t, [C.POINTER(RdecDesc)]),
    'vqvae_rdec_embed': (c_int, [C.POINTER(RdecDesc), C.POINTER(RdecTables), P, P, P, P, P]),
    'vqvae_rdec_cond_project': (c_int, [C.POINTER(RdecDesc), C.POINTER(RdecTables), P, P, P, P]),
    'vqvae_rdec_cond_global': (c_int, [C.POINTER(RdecDesc), P, P, P, P, P]),
    'vqvae_rdec_gate': (c_int, [C.POINTER(RdecDesc), C.POINTER(RdecTables), c_int, c_int, P, P, P, P, P, P]),
    'vqvae_rdec_res_skip': (c_int, [C.POINTER(RdecDesc), P, P, P, P, P, P, P, P, c_int, P]),
    'vqvae_rdec_head': (c_int, [C.POINTER(RdecDesc), C.POINTER(RdecTables), P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    'vqvae_rdec_reduce': (c_int, [C.POINTER(RdecDesc), C.POINTER(RdecTables), P, P, P, P, P]),
})
RAGGED_DECODER_MAX_CLASSES = 512
RAGGED_DECODER_MAX_DILATION = 512
RAGGED_DECODER_REDUCE_LANES = 256

# include/vqvae_align.h: dynamic time warping over mel-cepstra for a ragged list of utterance pairs
_header('vqvae_align.h', 'alignment ABI', 1, {
    'vqvae_align_abi_version': (c_int, []),
    'vqvae_align_cepstra_workspace_bytes': (c_size_t, [C.POINTER(AlignDesc)]),
    'vqvae_align_dtw_workspace_bytes': (c_size_t, [C.POINTER(AlignDesc)]),
    'vqvae_align_path_workspace_bytes': (c_size_t, [C.POINTER(AlignDesc)]),
    'vqvae_align_cepstra': (c_int, [C.POINTER(AlignDesc), c_int, P, P, P, P, c_size_t, P]),
    'vqvae_align_dtw': (c_int, [C.POINTER(AlignDesc), C.POINTER(AlignTables), P, P, P, P, P, P, c_size_t, P]),
    'vqvae_align_path': (c_int, [C.POINTER(AlignDesc), C.POINTER(AlignTables), P, P, P, P, P, P, P, P, P, c_size_t, P]),
})
ALIGN_MAX_SHORT = 3072
ALIGN_MAX_MELS = 128
ALIGN_THREADS = 256
ALIGN_REDUCE_LANES = 256

# include/vqvae_codes.h: runs, per-speaker counts and the edit distance of the discrete codes of a ragged list
_header('vqvae_codes.h', 'code-statistics ABI', 1, {
    'vqvae_codes_abi_version': (c_int, []),
    'vqvae_codes_runs_workspace_bytes': (c_size_t, [C.POINTER(CodesRunsDesc)]),
    'vqvae_codes_hist_workspace_bytes': (c_size_t, [C.POINTER(CodesHistDesc)]),
    'vqvae_codes_agree_workspace_bytes': (c_size_t, [C.POINTER(CodesPairDesc)]),
    'vqvae_codes_edit_workspace_bytes': (c_size_t, [C.POINTER(CodesPairDesc)]),
    'vqvae_codes_runs': (c_int, [C.POINTER(CodesRunsDesc), P, P, P, P, P, P, P, P, c_size_t, P]),
    'vqvae_codes_hist': (c_int, [C.POINTER(CodesHistDesc), P, P, P, P, P, P, P, P, c_size_t, P]),
    'vqvae_codes_agree': (c_int, [C.POINTER(CodesPairDesc), C.POINTER(CodesPairTables), P, P, P, P, c_size_t, P]),
    'vqvae_codes_edit': (c_int, [C.POINTER(CodesPairDesc), C.POINTER(CodesPairTables), P, P, P, P, P, c_size_t, P]),
})
CODES_MAX_SHORT = 6143
CODES_THREADS = 256
CODES_MAX_BIGRAM_K = 4096

PROTOTYPES = HEADERS['vqvae_hip.h'].prototypes
ABI_VERSION = HEADERS['vqvae_hip.h'].version
MAX_STACK_GROUP = 24
# upper-case integers that mirror no macro of a public header, and why
UNMIRRORED = (('ABI_VERSION', "the version HEADERS['vqvae_hip.h'] binds, not a macro"),
              ('MAX_STACK_GROUP', 'blocks per resstack call: MAXSEG of csrc/gemm_common.h, a private header'))

# include/vqvae_hip.h: storage bits, elementwise op codes, profiler tags, sampling modes
STORE_X_BF16, STORE_RES_BF16 = 2, 4
STORE_GX_BF16, STORE_GRES_BF16 = 8, 16
STORE_GH_BF16 = 1                 # vqvae_resblock_desc.storage bits (VQVAE_STORE_*)
STORE_GH_F16X2, STORE_X_F16X2, STORE_RES_F16X2 = 32, 64, 128      # matmul mode 3: kept pre-split (fp16 hi | lo dwords)
STORE_GATES_SIG = 256         # matmul mode 3: the gate kernel saves sigmoid and z only, the backward takes tanh = z / sigmoid
AMAX_SLOTS = 16                   # uint32 words per absolute maximum (vqvae_absmax, vqvae_resblock_amax)
EW_ADD, EW_SUB, EW_MUL, EW_AXPBY, EW_SCALE, EW_SQUARE, EW_RELU, EW_RELU_BWD, EW_FILL, \
    EW_MUL_SCALAR_DEV = range(10)
PROF_RESBLOCK_GATE, PROF_RESBLOCK_OUT, PROF_RESBLOCK_BWD_GZ, PROF_RESBLOCK_BWD_GX, \
    PROF_RESBLOCK_BWD_GC, PROF_RESBLOCK_WGRAD, PROF_CONV_FWD, PROF_CONV_BWD_DATA, \
    PROF_CONV_WGRAD, PROF_VQ_NEAREST, PROF_RESSTACK_SKIP, PROF_WGRAD_DIL, PROF_WGRAD_RES_SKIP = range(1, 14)
# vqvae_conv1d_forms: the bits of its word (VQVAE_CONV_FORM_*) and the family values (VQVAE_CONV_GEMM_* / _WGRAD_*)
CONV_FORM_FAMILY, CONV_FORM_ROWS256, CONV_FORM_WIDE, CONV_FORM_NP, CONV_FORM_NP_SHIFT = 0x003, 0x004, 0x008, 0x030, 4
CONV_FORM_TAP2, CONV_FORM_LEAN, CONV_FORM_HALVED, CONV_FORM_SPLIT, CONV_FORM_STRIDED, CONV_FORM_PHASES = \
    0x040, 0x080, 0x100, 0x200, 0x400, 0x800
CONV_GEMM_LIN128, CONV_GEMM_TILED, CONV_GEMM_FP32 = range(3)
CONV_WGRAD_W3, CONV_WGRAD_W2, CONV_WGRAD_GENERIC = range(3)
GEN_NONE, GEN_SOFTMAX, GEN_MOL = range(3)
GEN_MAX_N = 4               # VQVAE_GEN_MAX_N: the persistent kernel and WaveNet.initialize
GEN_MAX_LOCKSTEP = 128      # VQVAE_GEN_MAX_LOCKSTEP: vqvae_wavenet_gen_step


class HipError(RuntimeError):
    pass


_lib = None


def load():
    """Loads libvqvae_hip.so (once).  Raises loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libvqvae_hip.so not found at %s -- build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` (hipcc, gfx950). '
            'There is no CPU fallback.' % LIB_PATH)
    # the host driver only supports dmabuf IPC: RCCL's peer-memory exchange fails with the legacy mode.
    # Must be in the environment before the HSA runtime initialises (first HIP call).
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    lib = C.CDLL(LIB_PATH)
    for h in HEADERS.values():
        for name, (res, args) in h.prototypes.items():
            fn = getattr(lib, name)           # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
    for h in HEADERS.values():                # the ctypes structs above mirror ONE layout of each header
        has = getattr(lib, h.version_symbol)()
        if has != h.version:
            raise ImportError('libvqvae_hip.so at %s has %s %d, this package binds %s%d: rebuild it (__graft_entry__.build())'
                              % (LIB_PATH, h.words, has, 'ABI ' if h.file == 'vqvae_hip.h' else '', h.version))
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().vqvae_last_error_string()
        raise HipError('%s failed (code %d): %s' % (what or 'libvqvae_hip call', rc,
                                                    msg.decode() if msg else ''))


def call(name, *args):
    """Calls an int-returning entry point and raises HipError on failure."""
    check(getattr(load(), name)(*args), name)

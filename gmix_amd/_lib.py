"""ctypes binding of libgmxmix.so (include/gmxmix.h).  The library is the product: if it is
missing or cannot be loaded this module raises -- there is no Python or CPU fallback."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# GMX_LIB overrides the library file (an instrumented build of the same sources, for profiling)
LIB_PATH = os.environ.get("GMX_LIB") or os.path.join(_HERE, "libgmxmix.so")
_LIB = None


class GmxError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        L = _LIB
        msg = L.gmx_strerror(status).decode() if L else str(status)
        extra = L.gmx_last_error().decode() if (L and status == -3) else ""
        super().__init__(f"{where}: {msg} [{status}] {extra}".strip())


class MixerDesc(C.Structure):
    _fields_ = [("layer", C.c_int32), ("table_size", C.c_uint32), ("learning_rate", C.c_float)]


class IndirectDesc(C.Structure):
    _fields_ = [("table_size", C.c_uint32), ("learning_rate", C.c_float), ("slot_indirect", C.c_int32),
                ("slot_run_map", C.c_int32)]


class MatchDesc(C.Structure):
    _fields_ = [("table_size", C.c_uint32), ("limit", C.c_int32), ("slot", C.c_int32)]


class CtxDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32), ("num_bits", C.c_int32), ("n_bytes", C.c_int32),
                ("outer_order", C.c_int32), ("inner_order", C.c_int32), ("table_size", C.c_uint32),
                ("bytes_to_use", C.c_uint8 * 8), ("map", C.c_uint8 * 256)]


class CtxTargets(C.Structure):
    _fields_ = [("mixers", C.c_void_p), ("mixer_route", C.POINTER(C.c_int32)), ("n_mixer_route", C.c_int32),
                ("indirect", C.c_void_p), ("ind_route", C.POINTER(C.c_int32)), ("n_ind_route", C.c_int32),
                ("match", C.c_void_p), ("match_route", C.POINTER(C.c_int32)), ("n_match_route", C.c_int32)]


class CtxStepRoutes(C.Structure):
    _fields_ = [("mixer_route", C.POINTER(C.c_int32)), ("n_mixer_route", C.c_int32),
                ("ind_route", C.POINTER(C.c_int32)), ("n_ind_route", C.c_int32),
                ("match_route", C.POINTER(C.c_int32)), ("n_match_route", C.c_int32)]


class CtxBlackboard(C.Structure):
    _fields_ = [("recent_bits", C.c_int32), ("new_bit", C.c_int32), ("last_byte", C.c_uint32),
                ("rotating_history_pos", C.c_uint32), ("first_prediction", C.c_int32),
                ("recent_bytes", C.c_uint32 * 10), ("values", C.c_uint32 * 64), ("rotating_history", C.c_uint8 * 1000)]


class TopologyStruct(C.Structure):
    _fields_ = [("n_inputs", C.c_int32), ("n_skip", C.c_int32), ("skip_index", C.POINTER(C.c_int32)),
                ("n_mixers", C.c_int32), ("mixers", C.POINTER(MixerDesc))]


def build(force=False):
    """Compile libgmxmix.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", src, "clean"])
    subprocess.check_call(["make", "-s", "-C", src, "all"])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP extension is the only implementation; nothing falls back to CPU)")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32
    L.gmx_strerror.restype = C.c_char_p
    L.gmx_strerror.argtypes = [i32]
    L.gmx_last_error.restype = C.c_char_p
    L.gmx_build_info.restype = C.c_char_p
    L.gmx_device_count.argtypes = [C.POINTER(C.c_int)]
    L.gmx_device_pci_bus_id.argtypes = [i32, C.c_char_p, C.c_size_t]
    L.gmx_group_create.argtypes = [C.POINTER(vp), C.POINTER(TopologyStruct), i32, i32]
    L.gmx_group_destroy.argtypes = [vp]
    L.gmx_group_destroy.restype = None
    for f in (L.gmx_group_n_streams, L.gmx_group_n_mixers, L.gmx_group_n_inputs, L.gmx_group_reset,
              L.gmx_group_sync):
        f.argtypes = [vp]
    L.gmx_group_timer_start.argtypes = [vp]
    L.gmx_group_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    L.gmx_group_bank_bytes.argtypes = [vp]
    L.gmx_group_bank_bytes.restype = u64
    L.gmx_bank_forward.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(C.c_float), vp]
    L.gmx_bank_learn.argtypes = [vp, i32, i32]
    L.gmx_batch_create.argtypes = [C.POINTER(vp), vp, u64, C.c_uint]
    L.gmx_batch_destroy.argtypes = [vp]
    L.gmx_batch_destroy.restype = None
    L.gmx_batch_n_pad.argtypes = [vp]
    L.gmx_batch_mask_words.argtypes = [vp]
    L.gmx_batch_max_bits.argtypes = [vp]
    L.gmx_batch_max_bits.restype = u64
    for name in ("gmx_batch_predictions", "gmx_batch_active_mask", "gmx_batch_contexts",
                 "gmx_batch_bits", "gmx_batch_p", "gmx_batch_outputs", "gmx_batch_last_outputs"):
        f = getattr(L, name)
        f.argtypes = [vp]
        f.restype = vp
    L.gmx_batch_upload.argtypes = [vp, u64]
    L.gmx_batch_download.argtypes = [vp, u64]
    L.gmx_batch_wait.argtypes = [vp]
    L.gmx_batch_fill_synthetic.argtypes = [vp, u64, u64, u64, i32, u32, u32, i32]
    L.gmx_group_run.argtypes = [vp, vp, u64, i32, C.POINTER(C.c_float)]
    L.gmx_group_run_ragged.argtypes = [vp, vp, C.POINTER(u64), i32]
    L.gmx_topology_register_rows_eligible.argtypes = [C.POINTER(TopologyStruct)]
    L.gmx_group_set_register_rows.argtypes = [vp, i32]
    L.gmx_bank_export.argtypes = [vp, i32, vp, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_size_t)]
    L.gmx_bank_import.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t]
    L.gmx_bank_copy.argtypes = [vp, i32, vp, i32]
    L.gmx_group_export.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.gmx_group_import.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_size_t), vp]
    L.gmx_bank_memory_usage.argtypes = [vp, i32, i32, C.POINTER(u64)]
    L.gmx_indirect_create.argtypes = [C.POINTER(vp), C.POINTER(IndirectDesc), i32, vp, vp, i32, i32]
    L.gmx_indirect_destroy.argtypes = [vp]
    L.gmx_indirect_destroy.restype = None
    for f in (L.gmx_indirect_n_streams, L.gmx_indirect_n_models, L.gmx_indirect_reset, L.gmx_indirect_sync):
        f.argtypes = [vp]
    L.gmx_indirect_bank_bytes.argtypes = [vp]
    L.gmx_indirect_bank_bytes.restype = u64
    L.gmx_indirect_forward.argtypes = [vp, i32, vp, u32, vp, vp]
    L.gmx_chain_forward.argtypes = [vp, vp, i32, vp, u32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.gmx_indirect_attach_match.argtypes = [vp, vp, C.POINTER(C.c_int32), i32]
    L.gmx_chain_forward_match.argtypes = [vp, vp, i32, vp, vp, u32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gmx_indirect_learn.argtypes = [vp, i32, i32]
    L.gmx_ind_batch_create.argtypes = [C.POINTER(vp), vp, u64]
    L.gmx_ind_batch_destroy.argtypes = [vp]
    L.gmx_ind_batch_destroy.restype = None
    L.gmx_ind_batch_max_bits.argtypes = [vp]
    L.gmx_ind_batch_max_bits.restype = u64
    for name in ("gmx_ind_batch_contexts", "gmx_ind_batch_bit_contexts", "gmx_ind_batch_bits",
                 "gmx_ind_batch_predictions", "gmx_ind_batch_active"):
        f = getattr(L, name)
        f.argtypes = [vp]
        f.restype = vp
    L.gmx_ind_batch_upload.argtypes = [vp, u64]
    L.gmx_ind_batch_download.argtypes = [vp, u64]
    L.gmx_ind_batch_wait.argtypes = [vp]
    L.gmx_ind_batch_fill_synthetic.argtypes = [vp, u64, u64, u64, vp]
    L.gmx_indirect_run.argtypes = [vp, vp, u64, i32, vp, C.POINTER(C.c_float)]
    L.gmx_indirect_run_ragged.argtypes = [vp, vp, C.POINTER(u64), i32, vp]
    L.gmx_indirect_export.argtypes = [vp, i32, vp, C.POINTER(C.c_size_t)]
    L.gmx_indirect_import.argtypes = [vp, i32, vp, C.c_size_t]
    L.gmx_indirect_copy.argtypes = [vp, i32, vp, i32]
    L.gmx_indirect_group_export.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.gmx_indirect_group_import.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_size_t)]
    L.gmx_indirect_memory_usage.argtypes = [vp, i32, C.POINTER(u64)]
    L.gmx_indirect_slots_get.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.gmx_indirect_slots_set.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.gmx_lstm_create.argtypes = [C.POINTER(vp), i32, i32]
    L.gmx_lstm_destroy.argtypes = [vp]
    L.gmx_lstm_destroy.restype = None
    for f in (L.gmx_lstm_n_streams, L.gmx_lstm_reset, L.gmx_lstm_sync):
        f.argtypes = [vp]
    L.gmx_lstm_bank_bytes.argtypes = [vp]
    L.gmx_lstm_bank_bytes.restype = u64
    L.gmx_lstm_set_weights.argtypes = [vp, i32, vp]
    L.gmx_lstm_get_weights.argtypes = [vp, i32, vp, vp]
    L.gmx_lstm_batch_create.argtypes = [C.POINTER(vp), vp, u64]
    L.gmx_lstm_batch_destroy.argtypes = [vp]
    L.gmx_lstm_batch_destroy.restype = None
    for name in ("gmx_lstm_batch_ppm", "gmx_lstm_batch_bytes", "gmx_lstm_batch_predictions",
                 "gmx_lstm_batch_active", "gmx_lstm_batch_contexts"):
        f = getattr(L, name)
        f.argtypes = [vp]
        f.restype = vp
    L.gmx_lstm_batch_upload.argtypes = [vp, u64]
    L.gmx_lstm_batch_download.argtypes = [vp, u64]
    L.gmx_lstm_batch_wait.argtypes = [vp]
    L.gmx_lstm_run.argtypes = [vp, vp, u64, i32, C.POINTER(C.c_float)]
    L.gmx_lstm_run_ragged.argtypes = [vp, vp, C.POINTER(u64), i32]
    L.gmx_lstm_forward.argtypes = [vp, i32, i32, vp, vp, C.POINTER(u32)]
    L.gmx_lstm_perceive.argtypes = [vp, i32, i32]
    L.gmx_lstm_feed.argtypes = [vp, vp, u64, vp, i32, i32, vp, i32]
    L.gmx_lstm_export.argtypes = [vp, i32, vp, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_size_t)]
    L.gmx_lstm_import.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t]
    L.gmx_lstm_copy.argtypes = [vp, i32, vp, i32]
    L.gmx_lstm_memory_usage.argtypes = [vp, C.POINTER(u64)]
    L.gmx_lstm_group_export.argtypes = [vp, i32, i32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_size_t)]
    L.gmx_lstm_group_import.argtypes = [vp, i32, i32, vp, C.c_size_t, vp, C.c_size_t]
    L.gmx_match_create.argtypes = [C.POINTER(vp), C.POINTER(MatchDesc), i32, u64, i32, i32]
    L.gmx_match_destroy.argtypes = [vp]
    L.gmx_match_destroy.restype = None
    for f in (L.gmx_match_n_streams, L.gmx_match_n_models, L.gmx_match_reset, L.gmx_match_sync):
        f.argtypes = [vp]
    L.gmx_match_bank_bytes.argtypes = [vp]
    L.gmx_match_bank_bytes.restype = u64
    L.gmx_match_batch_create.argtypes = [C.POINTER(vp), vp, u64]
    L.gmx_match_batch_destroy.argtypes = [vp]
    L.gmx_match_batch_destroy.restype = None
    L.gmx_match_batch_max_bits.argtypes = [vp]
    L.gmx_match_batch_max_bits.restype = u64
    for name in ("contexts", "bit_contexts", "bits", "predictions", "active", "longest"):
        f = getattr(L, "gmx_match_batch_" + name)
        f.argtypes = [vp]
        f.restype = vp
    L.gmx_match_batch_upload.argtypes = [vp, u64]
    L.gmx_match_batch_download.argtypes = [vp, u64]
    L.gmx_match_batch_wait.argtypes = [vp]
    L.gmx_match_run.argtypes = [vp, vp, u64, vp, C.POINTER(C.c_int32), i32, C.POINTER(C.c_float)]
    L.gmx_match_run_ragged.argtypes = [vp, vp, C.POINTER(u64), vp, C.POINTER(C.c_int32), i32]
    L.gmx_match_forward.argtypes = [vp, i32, vp, u32, vp, vp, C.POINTER(u32)]
    L.gmx_match_learn.argtypes = [vp, i32, i32]
    L.gmx_match_slots_get.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.gmx_match_slots_set.argtypes = [vp, i32, C.POINTER(C.c_float), i32]
    L.gmx_match_history_size.argtypes = [vp, i32, C.POINTER(u64)]
    L.gmx_match_export.argtypes = [vp, i32, vp, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_size_t)]
    L.gmx_match_import.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t]
    L.gmx_match_copy.argtypes = [vp, i32, vp, i32]
    L.gmx_match_group_export.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.gmx_match_group_import.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_size_t), vp]
    L.gmx_match_memory_usage.argtypes = [vp, i32, C.POINTER(u64)]
    L.gmx_ctx_create.argtypes = [C.POINTER(vp), C.POINTER(CtxDesc), i32, i32, i32]
    L.gmx_ctx_destroy.argtypes = [vp]
    L.gmx_ctx_destroy.restype = None
    for f in (L.gmx_ctx_n_streams, L.gmx_ctx_n_vars, L.gmx_ctx_reset, L.gmx_ctx_sync):
        f.argtypes = [vp]
    L.gmx_ctx_bank_bytes.argtypes = [vp]
    L.gmx_ctx_bank_bytes.restype = u64
    L.gmx_ctx_set_cu_mask.argtypes = [vp, C.POINTER(u32), i32]
    L.gmx_ctx_batch_create.argtypes = [C.POINTER(vp), vp, u64, C.c_uint]
    L.gmx_ctx_batch_destroy.argtypes = [vp]
    L.gmx_ctx_batch_destroy.restype = None
    L.gmx_ctx_batch_max_bits.argtypes = [vp]
    L.gmx_ctx_batch_max_bits.restype = u64
    for name in ("bits", "values"):
        f = getattr(L, "gmx_ctx_batch_" + name)
        f.argtypes = [vp]
        f.restype = vp
    L.gmx_ctx_batch_upload.argtypes = [vp, u64]
    L.gmx_ctx_batch_download.argtypes = [vp, u64]
    L.gmx_ctx_batch_wait.argtypes = [vp]
    L.gmx_ctx_run.argtypes = [vp, vp, u64, C.POINTER(CtxTargets), C.POINTER(C.c_float)]
    L.gmx_ctx_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gmx_ctx_run_ragged.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(CtxTargets)]
    L.gmx_ctx_blackboard_get.argtypes = [vp, i32, C.POINTER(CtxBlackboard)]
    L.gmx_ctx_blackboard_set.argtypes = [vp, i32, C.POINTER(CtxBlackboard)]
    L.gmx_ctx_export.argtypes = [vp, i32, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.gmx_ctx_import.argtypes = [vp, i32, vp, C.c_size_t]
    L.gmx_ctx_copy.argtypes = [vp, i32, vp, i32]
    L.gmx_ctx_group_export.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.gmx_ctx_group_import.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_size_t)]
    L.gmx_ctx_group_blackboard_get.argtypes = [vp, i32, i32, C.POINTER(CtxBlackboard)]
    L.gmx_ctx_group_blackboard_set.argtypes = [vp, i32, i32, C.POINTER(CtxBlackboard)]
    L.gmx_debug_ctx_group_ops.argtypes = [vp]
    L.gmx_ctx_memory_usage.argtypes = [vp, i32, C.POINTER(u64)]
    L.gmx_chainstep_attach_ctx.argtypes = [vp, vp, C.POINTER(CtxStepRoutes)]
    L.gmx_chainstep_commit_bytes.argtypes = [vp]
    L.gmx_chainstep_commit_bytes.restype = u64
    L.gmx_chainstep_timed_step.argtypes = [vp, C.POINTER(C.c_float)]
    L.gmx_ctx_learn.argtypes = [vp, i32, i32]
    L.gmx_ctx_forward.argtypes = [vp, i32, vp, C.POINTER(u32)]
    L.gmx_indirect_attach_ctx.argtypes = [vp, vp, C.POINTER(CtxStepRoutes)]
    L.gmx_chain_forward_ctx.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gmx_lockstep_create.argtypes = [C.POINTER(vp), vp, C.c_uint]
    L.gmx_lockstep_destroy.argtypes = [vp]
    L.gmx_lockstep_destroy.restype = None
    L.gmx_lockstep_batch.argtypes = [vp]
    L.gmx_lockstep_batch.restype = vp
    L.gmx_lockstep_predict.argtypes = [vp]
    L.gmx_lockstep_is_persistent.argtypes = [vp]
    L.gmx_lockstep_learn.argtypes = [vp]
    L.gmx_lockstep_learn_predict.argtypes = [vp]
    L.gmx_chainstep_create.argtypes = [C.POINTER(vp), vp, vp, vp, i32, i32, i32]
    L.gmx_chainstep_destroy.argtypes = [vp]
    L.gmx_chainstep_destroy.restype = None
    L.gmx_chainstep_n_streams.argtypes = [vp]
    L.gmx_chainstep_step.argtypes = [vp]
    L.gmx_chainstep_commit.argtypes = [vp, i32]
    L.gmx_chainstep_launch.argtypes = [vp]
    L.gmx_chainstep_wait.argtypes = [vp]
    L.gmx_chainstep_attach_match.argtypes = [vp, vp, C.POINTER(C.c_int32), i32]
    for name in ("predictions", "active_mask", "contexts", "ind_contexts", "bit_contexts", "ppm", "bits", "what", "p",
                 "outputs", "match_contexts"):
        f = getattr(L, "gmx_chainstep_" + name)
        f.argtypes = [vp]
        f.restype = vp
    for name in ("gmx_group_set_cu_mask", "gmx_indirect_set_cu_mask", "gmx_lstm_set_cu_mask", "gmx_match_set_cu_mask"):
        getattr(L, name).argtypes = [vp, C.POINTER(u32), i32]
    if hasattr(L, "gmx_chainstep_attach_decoder"):
        # (include/gmxmix_decoder.h; an older build loaded through GMX_LIB for a comparison lacks them, and a call fails)
        L.gmx_chainstep_attach_decoder.argtypes = [vp, i32]
        L.gmx_chainstep_decoder_set_input.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(u32)]
        L.gmx_chainstep_decoder_state.argtypes = [vp, i32, C.POINTER(u32)]
        for name in ("byte", "byte_launch", "byte_wait"):
            getattr(L, "gmx_chainstep_" + name).argtypes = [vp]
        L.gmx_chainstep_timed_byte.argtypes = [vp, C.POINTER(C.c_float)]
        for name in ("decoder_ppm", "take", "decoded", "byte_p"):
            f = getattr(L, "gmx_chainstep_" + name)
            f.argtypes = [vp]
            f.restype = vp
        L.gmx_debug_chainstep_bit_launches.argtypes = [vp]
        L.gmx_debug_chainstep_bit_launches.restype = C.c_int64
    if hasattr(L, "gmx_lstm_create_shaped"):
        # (include/gmxmix_lstm_shape.h; an older build loaded through GMX_LIB for a comparison lacks them, and a call fails)
        L.gmx_lstm_shape_supported.argtypes = [C.POINTER(LstmShapeC)]
        L.gmx_lstm_create_shaped.argtypes = [C.POINTER(vp), C.POINTER(LstmShapeC), i32, i32]
        L.gmx_lstm_get_shape.argtypes = [vp, C.POINTER(LstmShapeC)]
        L.gmx_debug_lstm_any_launches.argtypes = [vp]
        L.gmx_debug_lstm_any_launches.restype = C.c_int64
    if hasattr(L, "gmx_encoder_create"):
        # (include/gmxmix_encoder.h; an older build loaded through GMX_LIB for a comparison lacks them, and a call fails)
        pu64 = C.POINTER(C.c_uint64)
        L.gmx_encoder_create.argtypes = [C.POINTER(vp), i32, u64, i32]
        L.gmx_encoder_destroy.argtypes = [vp]
        L.gmx_encoder_destroy.restype = None
        L.gmx_encoder_reset.argtypes = [vp, i32, C.POINTER(u32)]
        L.gmx_encoder_state.argtypes = [vp, i32, C.POINTER(u32)]
        L.gmx_encoder_encode_batch.argtypes = [vp, vp, pu64, C.POINTER(C.c_float)]
        L.gmx_encoder_encode.argtypes = [vp, vp, vp, u64, pu64]
        L.gmx_encoder_flush.argtypes = [vp, vp]
        for name in ("take", "take_launch", "take_wait"):
            getattr(L, "gmx_encoder_" + name).argtypes = [vp]
        L.gmx_encoder_bytes.argtypes = [vp, i32]
        L.gmx_encoder_bytes.restype = vp
        for name in ("n_bytes", "total_bytes"):
            f = getattr(L, "gmx_encoder_" + name)
            f.argtypes = [vp, i32]
            f.restype = C.c_uint64
        L.gmx_encoder_bad_bit.argtypes = [vp, i32]
        L.gmx_encoder_bad_bit.restype = C.c_int64
        L.gmx_debug_encoder_d2h_bytes.argtypes = [vp]
        L.gmx_debug_encoder_d2h_bytes.restype = C.c_int64
    if hasattr(L, "gmx_analysis_create"):
        # (include/gmxmix_analysis.h; an older build loaded through GMX_LIB for a comparison lacks them, and a call fails)
        pu64 = C.POINTER(C.c_uint64)
        L.gmx_analysis_create.argtypes = [C.POINTER(vp), i32, vp, i32, u64, i32]
        L.gmx_analysis_destroy.argtypes = [vp]
        L.gmx_analysis_destroy.restype = None
        L.gmx_analysis_reset.argtypes = [vp, i32, vp, u64]
        L.gmx_analysis_set_frequency.argtypes = [vp, i32, u64]
        L.gmx_analysis_update_batch.argtypes = [vp, vp, pu64, C.POINTER(C.c_float)]
        L.gmx_analysis_update.argtypes = [vp, vp, vp, u64, pu64]
        for name in ("take", "take_launch", "take_wait"):
            getattr(L, "gmx_analysis_" + name).argtypes = [vp]
        for name in ("ema", "samples", "sample_bits"):
            f = getattr(L, "gmx_analysis_" + name)
            f.argtypes = [vp, i32]
            f.restype = vp
        for name in ("bits_seen", "n_samples"):
            f = getattr(L, "gmx_analysis_" + name)
            f.argtypes = [vp, i32]
            f.restype = C.c_uint64
        L.gmx_debug_analysis_d2h_bytes.argtypes = [vp]
        L.gmx_debug_analysis_d2h_bytes.restype = C.c_int64
    if hasattr(L, "gmx_ppmd_create"):
        # (include/gmxmix_ppmd.h; an older build loaded through GMX_LIB for a comparison lacks them, and a call fails)
        L.gmx_ppmd_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32]
        L.gmx_ppmd_destroy.argtypes = [vp]
        L.gmx_ppmd_destroy.restype = None
        L.gmx_ppmd_n_streams.argtypes = [vp]
        L.gmx_ppmd_bank_bytes.argtypes = [vp]
        L.gmx_ppmd_bank_bytes.restype = u64
        L.gmx_ppmd_reset.argtypes = [vp, i32]
        L.gmx_ppmd_sync.argtypes = [vp]
        L.gmx_ppmd_batch_create.argtypes = [C.POINTER(vp), vp, u64]
        L.gmx_ppmd_batch_destroy.argtypes = [vp]
        L.gmx_ppmd_batch_destroy.restype = None
        L.gmx_ppmd_batch_max_bytes.argtypes = [vp]
        L.gmx_ppmd_batch_max_bytes.restype = u64
        for name in ("bytes", "ppm", "predictions", "active", "used"):
            f = getattr(L, "gmx_ppmd_batch_" + name)
            f.argtypes = [vp]
            f.restype = vp
        L.gmx_ppmd_batch_upload.argtypes = [vp, u64]
        L.gmx_ppmd_batch_download.argtypes = [vp, u64, C.c_uint]
        L.gmx_ppmd_batch_wait.argtypes = [vp]
        L.gmx_ppmd_run.argtypes = [vp, vp, u64, C.POINTER(C.c_float)]
        L.gmx_ppmd_run_ragged.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
        L.gmx_ppmd_feed.argtypes = [vp, vp, u64, vp, vp, i32]
        L.gmx_ppmd_step_launch.argtypes = [vp, vp, vp]
        L.gmx_ppmd_step_wait.argtypes = [vp]
        L.gmx_ppmd_step.argtypes = [vp, vp, vp]
        L.gmx_ppmd_step_ppm.argtypes = [vp]
        L.gmx_ppmd_step_ppm.restype = vp
        L.gmx_ppmd_memory_usage.argtypes = [vp, i32]
        L.gmx_ppmd_memory_usage.restype = u64
        L.gmx_ppmd_restores.argtypes = [vp, i32]
        L.gmx_ppmd_restores.restype = C.c_int64
        L.gmx_debug_ppmd_launches.argtypes = [vp]
        L.gmx_debug_ppmd_launches.restype = C.c_int64
    L.gmx_debug_math_probe.argtypes = [i32, vp, vp, u64, i32]
    L.gmx_debug_math_range.argtypes = [i32, u64, u64, i32, C.POINTER(C.c_ulonglong)]
    _LIB = L
    return L


class LstmShapeC(C.Structure):
    """gmx_lstm_shape of include/gmxmix_lstm_shape.h."""
    _fields_ = [("num_cells", C.c_int32), ("horizon", C.c_int32), ("learning_rate", C.c_float),
                ("gradient_clip", C.c_float)]


def check(status, where):
    if status != 0:
        raise GmxError(status, where)


# Every symbol include/gmxmix.h declares; tests assert the built library exports them all.
ABI_SYMBOLS = [
    "gmx_strerror", "gmx_last_error", "gmx_device_count", "gmx_device_pci_bus_id", "gmx_build_info", "gmx_group_create",
    "gmx_group_destroy", "gmx_group_n_streams", "gmx_group_n_mixers", "gmx_group_n_inputs",
    "gmx_group_bank_bytes", "gmx_group_reset", "gmx_group_sync", "gmx_group_timer_start", "gmx_group_timer_stop", "gmx_bank_forward", "gmx_bank_learn",
    "gmx_batch_create", "gmx_batch_destroy", "gmx_batch_n_pad", "gmx_batch_mask_words",
    "gmx_batch_max_bits", "gmx_batch_predictions", "gmx_batch_active_mask", "gmx_batch_contexts",
    "gmx_batch_bits", "gmx_batch_p", "gmx_batch_outputs", "gmx_batch_last_outputs", "gmx_batch_upload", "gmx_batch_download",
    "gmx_batch_wait", "gmx_batch_fill_synthetic", "gmx_group_run", "gmx_group_run_ragged",
    "gmx_topology_register_rows_eligible", "gmx_group_set_register_rows", "gmx_bank_export",
    "gmx_bank_import", "gmx_bank_copy", "gmx_group_export", "gmx_group_import", "gmx_bank_memory_usage",
    "gmx_lockstep_create", "gmx_lockstep_destroy", "gmx_lockstep_batch", "gmx_lockstep_is_persistent", "gmx_lockstep_predict", "gmx_lockstep_learn", "gmx_lockstep_learn_predict",
    "gmx_indirect_create", "gmx_indirect_destroy", "gmx_indirect_n_streams", "gmx_indirect_n_models",
    "gmx_indirect_bank_bytes", "gmx_indirect_reset", "gmx_indirect_sync", "gmx_indirect_forward", "gmx_chain_forward",
    "gmx_indirect_learn", "gmx_ind_batch_create", "gmx_ind_batch_destroy", "gmx_ind_batch_max_bits",
    "gmx_ind_batch_contexts", "gmx_ind_batch_bit_contexts", "gmx_ind_batch_bits",
    "gmx_ind_batch_predictions", "gmx_ind_batch_active", "gmx_ind_batch_upload", "gmx_ind_batch_download",
    "gmx_ind_batch_wait", "gmx_ind_batch_fill_synthetic", "gmx_indirect_run", "gmx_indirect_run_ragged", "gmx_indirect_export",
    "gmx_indirect_import", "gmx_indirect_copy", "gmx_indirect_group_export", "gmx_indirect_group_import", "gmx_indirect_memory_usage", "gmx_indirect_slots_get", "gmx_indirect_slots_set",
    "gmx_lstm_create", "gmx_lstm_destroy", "gmx_lstm_n_streams", "gmx_lstm_bank_bytes", "gmx_lstm_reset",
    "gmx_lstm_sync", "gmx_lstm_set_weights", "gmx_lstm_get_weights", "gmx_lstm_batch_create",
    "gmx_lstm_batch_destroy", "gmx_lstm_batch_ppm", "gmx_lstm_batch_bytes", "gmx_lstm_batch_predictions",
    "gmx_lstm_batch_active", "gmx_lstm_batch_contexts", "gmx_lstm_batch_upload", "gmx_lstm_batch_download",
    "gmx_lstm_batch_wait", "gmx_lstm_run", "gmx_lstm_run_ragged", "gmx_lstm_forward", "gmx_lstm_perceive", "gmx_lstm_feed",
    "gmx_lstm_export", "gmx_lstm_import", "gmx_lstm_copy", "gmx_lstm_memory_usage",
    "gmx_chainstep_create", "gmx_chainstep_destroy", "gmx_chainstep_n_streams", "gmx_chainstep_predictions",
    "gmx_chainstep_active_mask", "gmx_chainstep_contexts", "gmx_chainstep_ind_contexts", "gmx_chainstep_bit_contexts",
    "gmx_chainstep_ppm", "gmx_chainstep_bits", "gmx_chainstep_what", "gmx_chainstep_p", "gmx_chainstep_outputs",
    "gmx_chainstep_commit", "gmx_chainstep_step", "gmx_chainstep_launch", "gmx_chainstep_wait",
    "gmx_chainstep_attach_match", "gmx_chainstep_match_contexts",
    "gmx_indirect_attach_match", "gmx_chain_forward_match",
    "gmx_group_set_cu_mask", "gmx_indirect_set_cu_mask", "gmx_lstm_set_cu_mask",
    "gmx_match_create", "gmx_match_destroy", "gmx_match_n_streams", "gmx_match_n_models", "gmx_match_bank_bytes",
    "gmx_match_reset", "gmx_match_sync", "gmx_match_set_cu_mask", "gmx_match_batch_create", "gmx_match_batch_destroy",
    "gmx_match_batch_max_bits", "gmx_match_batch_contexts", "gmx_match_batch_bit_contexts", "gmx_match_batch_bits",
    "gmx_match_batch_predictions", "gmx_match_batch_active", "gmx_match_batch_longest", "gmx_match_batch_upload",
    "gmx_match_batch_download", "gmx_match_batch_wait", "gmx_match_run", "gmx_match_run_ragged", "gmx_match_forward",
    "gmx_match_learn", "gmx_match_slots_get", "gmx_match_slots_set", "gmx_match_history_size", "gmx_match_export",
    "gmx_match_import", "gmx_match_copy", "gmx_match_memory_usage", "gmx_match_group_export", "gmx_match_group_import",
    "gmx_ctx_create", "gmx_ctx_destroy", "gmx_ctx_n_streams", "gmx_ctx_n_vars", "gmx_ctx_bank_bytes", "gmx_ctx_reset",
    "gmx_ctx_sync", "gmx_ctx_set_cu_mask", "gmx_ctx_batch_create", "gmx_ctx_batch_destroy", "gmx_ctx_batch_max_bits",
    "gmx_ctx_batch_bits", "gmx_ctx_batch_values", "gmx_ctx_batch_upload", "gmx_ctx_batch_download",
    "gmx_ctx_batch_wait", "gmx_ctx_run", "gmx_ctx_run_ragged", "gmx_ctx_blackboard_get", "gmx_ctx_blackboard_set",
    "gmx_ctx_export", "gmx_ctx_import", "gmx_ctx_copy", "gmx_ctx_memory_usage", "gmx_ctx_last_kernel_ms",
    "gmx_chainstep_attach_ctx", "gmx_chainstep_commit_bytes", "gmx_chainstep_timed_step",
    "gmx_ctx_group_export", "gmx_ctx_group_import", "gmx_ctx_group_blackboard_get", "gmx_ctx_group_blackboard_set",
    "gmx_debug_ctx_group_ops",
    "gmx_ctx_learn", "gmx_ctx_forward", "gmx_indirect_attach_ctx", "gmx_chain_forward_ctx",
]

# What include/gmxmix_lstm_group.h declares on top of that: the extension header's symbols, exported by the same library
# (ABI_SYMBOLS mirrors include/gmxmix.h alone; its length is pinned by tests/test_chain_ctx_abi.py).
ABI_SYMBOLS_LSTM_GROUP = ["gmx_lstm_group_export", "gmx_lstm_group_import"]

# What include/gmxmix_decoder.h declares: a whole byte per call in the lock-step chain.
ABI_SYMBOLS_DECODER = [
    "gmx_chainstep_attach_decoder", "gmx_chainstep_decoder_ppm", "gmx_chainstep_decoder_set_input",
    "gmx_chainstep_decoder_state", "gmx_chainstep_take", "gmx_chainstep_byte", "gmx_chainstep_byte_launch",
    "gmx_chainstep_byte_wait", "gmx_chainstep_timed_byte", "gmx_chainstep_decoded", "gmx_chainstep_byte_p",
    "gmx_debug_chainstep_bit_launches",
]

# What include/gmxmix_lstm_shape.h declares: an LSTM bank of any width and horizon.
ABI_SYMBOLS_LSTM_SHAPE = [
    "gmx_lstm_shape_supported", "gmx_lstm_create_shaped", "gmx_lstm_get_shape", "gmx_debug_lstm_any_launches",
]

# What include/gmxmix_encoder.h declares: the arithmetic encoder on the device.
ABI_SYMBOLS_ENCODER = [
    "gmx_encoder_create", "gmx_encoder_destroy", "gmx_encoder_reset", "gmx_encoder_state", "gmx_encoder_encode_batch",
    "gmx_encoder_encode", "gmx_encoder_flush", "gmx_encoder_take", "gmx_encoder_take_launch", "gmx_encoder_take_wait",
    "gmx_encoder_bytes", "gmx_encoder_n_bytes", "gmx_encoder_total_bytes", "gmx_encoder_bad_bit",
    "gmx_debug_encoder_d2h_bytes",
]

# What include/gmxmix_analysis.h declares: the analysis averages on the device.
ABI_SYMBOLS_ANALYSIS = [
    "gmx_analysis_create", "gmx_analysis_destroy", "gmx_analysis_reset", "gmx_analysis_set_frequency",
    "gmx_analysis_update_batch", "gmx_analysis_update", "gmx_analysis_take", "gmx_analysis_take_launch",
    "gmx_analysis_take_wait", "gmx_analysis_ema", "gmx_analysis_bits_seen", "gmx_analysis_n_samples",
    "gmx_analysis_samples", "gmx_analysis_sample_bits", "gmx_debug_analysis_d2h_bytes",
]

# What include/gmxmix_ppmd.h declares: the PPMd byte model on the device.
ABI_SYMBOLS_PPMD = [
    "gmx_ppmd_create", "gmx_ppmd_destroy", "gmx_ppmd_n_streams", "gmx_ppmd_bank_bytes", "gmx_ppmd_reset", "gmx_ppmd_sync",
    "gmx_ppmd_batch_create", "gmx_ppmd_batch_destroy", "gmx_ppmd_batch_max_bytes", "gmx_ppmd_batch_bytes",
    "gmx_ppmd_batch_ppm", "gmx_ppmd_batch_predictions", "gmx_ppmd_batch_active", "gmx_ppmd_batch_used",
    "gmx_ppmd_batch_upload", "gmx_ppmd_batch_download", "gmx_ppmd_batch_wait", "gmx_ppmd_run", "gmx_ppmd_run_ragged",
    "gmx_ppmd_feed", "gmx_ppmd_step_launch", "gmx_ppmd_step_wait", "gmx_ppmd_step", "gmx_ppmd_step_ppm",
    "gmx_ppmd_memory_usage", "gmx_ppmd_restores", "gmx_debug_ppmd_launches",
]

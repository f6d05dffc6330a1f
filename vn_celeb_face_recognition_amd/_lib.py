"""ctypes binding of libvnface.so (include/vnface.h).  Fails loudly when the library is absent:
there is no CPU fallback on the product path."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvnface.so")

VNF_F32, VNF_BF16, VNF_F16, VNF_I64, VNF_U8, VNF_F16X2 = 0, 1, 2, 3, 4, 5
VNF_ARCH_IRV1, VNF_ARCH_IR100, VNF_ARCH_RN50_2B, VNF_ARCH_SEIR101 = 0, 1, 2, 3


class VnfError(RuntimeError):
    pass


class TensorDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("dtype", ctypes.c_int32),
                ("ndim", ctypes.c_int32), ("shape", ctypes.c_int64 * 4)]


class MtcnnCfg(ctypes.Structure):
    _fields_ = [("min_face_size", ctypes.c_int32), ("thresholds", ctypes.c_float * 3), ("factor", ctypes.c_float),
                ("select_largest", ctypes.c_int32), ("max_batch", ctypes.c_int32), ("max_height", ctypes.c_int32),
                ("max_width", ctypes.c_int32), ("max_candidates", ctypes.c_int32)]


class RetinaCfg(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int32), ("width", ctypes.c_int32), ("max_batch", ctypes.c_int32),
                ("conf_thres", ctypes.c_float), ("topk_bf_nms", ctypes.c_int32), ("nms_thres", ctypes.c_float),
                ("keep_top_k", ctypes.c_int32), ("vis_thres", ctypes.c_float), ("compute_dtype", ctypes.c_int32)]


class JpegInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32),
                ("sampling", ctypes.c_int32), ("h", ctypes.c_int32 * 3), ("v", ctypes.c_int32 * 3),
                ("restart_interval", ctypes.c_int32), ("blocks_w", ctypes.c_int32 * 3), ("blocks_h", ctypes.c_int32 * 3),
                ("quant", (ctypes.c_uint8 * 64) * 3), ("coef_count", ctypes.c_int64)]


class OverlayOp(ctypes.Structure):   # vnf_overlay_op
    _fields_ = [(k, ctypes.c_int32) for k in ("kind", "frame", "x0", "y0", "x1", "y1", "mask_offset")] + [("rgb", ctypes.c_uint32)]


class ConvProbeGeom(ctypes.Structure):   # vnf_conv_probe_geom
    _fields_ = ([(k, ctypes.c_int32) for k in ("n", "h", "w", "cin", "kh", "kw", "sh", "sw", "ph", "pw", "cout", "x_coff", "ldx", "nseg")] +
                [(k, ctypes.c_int32 * 4) for k in ("seg_c0", "seg_c1", "seg_ld", "seg_coff")] +
                [(k, ctypes.c_int32) for k in ("has_res", "ldres", "res_coff", "act", "out_f32", "dtype", "planar")])


_lib = None

# every symbol include/vnface.h declares, with its ctypes signature
_P = ctypes.c_void_p
_I = ctypes.c_int
SIGNATURES = {
    "vnf_init": (_I, [_I]),
    "vnf_last_error": (ctypes.c_char_p, []),
    "vnf_version": (ctypes.c_char_p, []),
    "vnf_destroy": (_I, [_P]),
    "vnf_encoder_create": (_I, [_I, ctypes.POINTER(TensorDesc), _I, _I, _I, ctypes.POINTER(_P)]),
    "vnf_embed": (_I, [_P, _P, _I, _I, _P, _P]),
    "vnf_encoder_tap": (_I, [_P, ctypes.c_char_p, _I, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "vnf_encoder_profile": (_I, [_P, _P, _I, _I, _P, _P, ctypes.c_char_p, ctypes.c_int64]),
    "vnf_encoder_flops": (_I, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "vnf_encoder_set_streams": (_I, [_P, _I]),
    "vnf_encoder_set_contexts": (_I, [_P, _I]),
    "vnf_encoder_create_classifier": (_I, [_I, ctypes.POINTER(TensorDesc), _I, _I, _I, _I, ctypes.POINTER(_P)]),
    "vnf_encoder_logprobs": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "vnf_logits_eval": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vnf_emotion_create": (_I, [ctypes.POINTER(TensorDesc), _I, _I, _I, _I, _I, ctypes.POINTER(_P)]),
    "vnf_emotion_forward": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "vnf_emotion_recognize": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "vnf_emotion_prep": (_I, [_P, _I, _I, _P, _I, _P]),
    "vnf_augment_faces": (_I, [_P, _I, _I, _P, _P, _I, _I, _P, _I, _P, _P]),
    "vnf_softmax_topk": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "vnf_maxpool3s2p1": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "vnf_se_block": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, ctypes.c_float, _P, _P, ctypes.c_float, _P, _P]),
    "vnf_conv_probe_create": (_I, [ctypes.POINTER(ConvProbeGeom), _P, _P, _P, _P, _P, ctypes.POINTER(_P)]),
    "vnf_conv_probe_cfgs": (_I, [_P, ctypes.POINTER(ctypes.c_int32), _I, ctypes.POINTER(ctypes.c_int32)]),
    "vnf_conv_cfg_tile": (_I, [_I, ctypes.POINTER(ctypes.c_int32)]),
    "vnf_conv_probe_run": (_I, [_P, _I, _P, ctypes.POINTER(_P), _P, _P]),
    "vnf_mlp_create": (_I, [ctypes.POINTER(TensorDesc), _I, _I, _I, _I, ctypes.POINTER(_P)]),
    "vnf_classify": (_I, [_P, _P, _I, _P, _P, _P, _P]),
    "vnf_mlp_trainer_create": (_I, [ctypes.POINTER(TensorDesc), _I, _I, _I, _I, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                   ctypes.c_float, ctypes.POINTER(_P)]),
    "vnf_mlp_train_step": (_I, [_P, _P, _P, _I, _P, ctypes.c_float, _I, _P, _P, _P]),
    "vnf_trainer_get": (_I, [_P, ctypes.c_char_p, _I, _P, ctypes.c_int64]),
    "vnf_trainer_set": (_I, [_P, ctypes.c_char_p, _I, _P, ctypes.c_int64]),
    "vnf_trainer_step_count": (_I, [_P, ctypes.POINTER(ctypes.c_int64), _I]),
    "vnf_encoder_features": (_I, [_P, _P, _I, _I, _P, _P]),
    "vnf_head_trainer_create": (_I, [ctypes.POINTER(TensorDesc), _I, _I, _I, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_float, ctypes.POINTER(_P)]),
    "vnf_head_train_step": (_I, [_P, _P, _P, _I, ctypes.c_float, _I, _P, _P, _P]),
    "vnf_mtcnn_create": (_I, [ctypes.POINTER(TensorDesc), _I, ctypes.POINTER(TensorDesc), _I,
                              ctypes.POINTER(TensorDesc), _I, ctypes.POINTER(MtcnnCfg), ctypes.POINTER(_P)]),
    "vnf_mtcnn_detect": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, ctypes.POINTER(ctypes.c_int32), _P]),
    "vnf_mtcnn_results_device": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "vnf_mtcnn_stage_times": (_I, [_P, _P, _I, _I, _I, ctypes.c_char_p, ctypes.c_int64, _P]),
    "vnf_mtcnn_debug_stage3": (_I, [_P, _P, _P, _I, _P, _I, ctypes.POINTER(ctypes.c_int32), _P]),
    "vnf_mtcnn_debug_pnet": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, ctypes.POINTER(ctypes.c_int32), _P]),
    "vnf_mtcnn_debug_net": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, ctypes.POINTER(ctypes.c_int32), _P]),
    "vnf_mtcnn_debug_net_tap": (_I, [_P, _I, ctypes.c_char_p, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]),
    "vnf_retina_create": (_I, [ctypes.POINTER(TensorDesc), _I, ctypes.POINTER(RetinaCfg), ctypes.POINTER(_P)]),
    "vnf_retina_detect": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, ctypes.POINTER(ctypes.c_int32), _P]),
    "vnf_retina_results_device": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "vnf_retina_debug_heads": (_I, [_P, _I, _I, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]),
    "vnf_align": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P]),
    "vnf_extract_faces": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _P, _I, _P, _P]),
    "vnf_jpeg_probe": (_I, [_P, ctypes.c_int64, ctypes.POINTER(JpegInfo)]),
    "vnf_jpeg_entropy_decode": (_I, [_P, ctypes.c_int64, ctypes.POINTER(JpegInfo), _P, ctypes.c_int64]),
    "vnf_jpeg_workspace_bytes": (ctypes.c_int64, [_I, _I, _I, _I]),
    "vnf_jpeg_decode_frames": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, ctypes.c_int64, _P]),
    "vnf_jpeg_quant_tables": (_I, [_I, _P, _P]),
    "vnf_jpeg_encode_info": (_I, [_I, _I, _I, _I, ctypes.POINTER(JpegInfo)]),
    "vnf_jpeg_encode_workspace_bytes": (ctypes.c_int64, [_I, _I, _I, _I]),
    "vnf_jpeg_encode_frames": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "vnf_jpeg_entropy_encode": (_I, [_P, ctypes.POINTER(JpegInfo), _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "vnf_jpeg_huff_header": (_I, [ctypes.POINTER(JpegInfo), _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "vnf_jpeg_huff_workspace_bytes": (ctypes.c_int64, [_I, ctypes.POINTER(JpegInfo), ctypes.c_int64]),
    "vnf_jpeg_huff_encode_frames": (_I, [_P, _I, ctypes.POINTER(JpegInfo), _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P,
                                        ctypes.c_int64, _P]),
    "vnf_jpeg_huff_prepared_bound": (ctypes.c_int64, [ctypes.c_int64, ctypes.POINTER(JpegInfo)]),
    "vnf_jpeg_huff_prepare": (_I, [_P, ctypes.c_int64, ctypes.POINTER(JpegInfo), _P, ctypes.c_int64,
                                  ctypes.POINTER(ctypes.c_int64)]),
    "vnf_jpeg_huff_decode_workspace_bytes": (ctypes.c_int64, [_I, ctypes.POINTER(JpegInfo), ctypes.c_int64, _I]),
    "vnf_jpeg_huff_decode_frames": (_I, [_P, _P, _P, _I, ctypes.POINTER(JpegInfo), _I, _P, _P, _P, ctypes.c_int64, _P]),
    "vnf_gallery_create": (_I, [_I, ctypes.c_int64, ctypes.POINTER(_P)]),
    "vnf_gallery_add": (_I, [_P, _P, _P, ctypes.c_int64, _P]),
    "vnf_gallery_add_unit": (_I, [_P, _P, _P, ctypes.c_int64, _P]),
    "vnf_gallery_rows": (_I, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P]),
    "vnf_gallery_size": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "vnf_gallery_class_sums": (_I, [_P, _P, ctypes.c_int64, _I, _P, _P, _I, _P]),
    "vnf_gallery_search_workspace_bytes": (ctypes.c_int64, [_I, _I, ctypes.c_int64, ctypes.c_int64]),
    "vnf_gallery_search": (_I, [_P, _P, _I, _I, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    "vnf_gallery_mated_search_workspace_bytes": (ctypes.c_int64, [_I, ctypes.c_int64, ctypes.c_int64]),
    "vnf_gallery_mated_search": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    "vnf_gallery_cluster_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "vnf_gallery_cluster": (_I, [_P, ctypes.c_float, _I, _P, _P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    "vnf_gallery_tracks_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "vnf_gallery_tracks": (_I, [_P, _P, _I, _P, ctypes.c_float, ctypes.c_float, _I, _P, _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "vnf_gallery_track_sums": (_I, [_P, _P, _P, _P, _I, _P, _P, _P]),
    "vnf_overlay_draw": (_I, [_P, _I, _I, _I, _P, _I, _P, ctypes.c_int64, _P]),
    "vnf_overlay_draw_text": (_I, [_P, _I, _I, _I, _P, _I, _P, _I, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
}


def load():
    """Load (once) and return the ctypes library.  Raises VnfError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VnfError("libvnface.so is not built (%s): run `python -m vn_celeb_face_recognition_amd.build` "
                       "or __graft_entry__.build().  There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise VnfError("libvnface error %d: %s" % (rc, load().vnf_last_error().decode("utf-8", "replace")))


def workspace(nbytes, device):
    """What a vnf_*_workspace_bytes call answered -> the uint8 scratch tensor on `device`; a negative answer is the
    library's error code and raises it."""
    import torch
    if nbytes < 0:
        check(int(nbytes))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def make_descs(state_dict):
    """state_dict (name -> torch.Tensor | ndarray) -> (TensorDesc array, keepalive list)."""
    import torch
    items = []
    keep = []
    for name, v in state_dict.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu()
            if not v.dtype.is_floating_point:
                continue
            a = v.float().contiguous().numpy()
        else:
            a = np.asarray(v)
            if a.dtype.kind != "f":
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim > 4:
            raise VnfError("tensor %s has more than 4 dims" % name)
        keep.append(a)
        items.append((name.encode(), a))
    arr = (TensorDesc * len(items))()
    for i, (nm, a) in enumerate(items):
        keep.append(nm)
        arr[i].name = nm
        arr[i].data = a.ctypes.data
        arr[i].dtype = VNF_F32
        arr[i].ndim = a.ndim
        for d in range(a.ndim):
            arr[i].shape[d] = a.shape[d]
    return arr, len(items), keep


_TORCH_DT = None


def torch_dtype_code(dt):
    import torch
    global _TORCH_DT
    if _TORCH_DT is None:
        _TORCH_DT = {torch.float32: VNF_F32, torch.bfloat16: VNF_BF16, torch.float16: VNF_F16}
    if dt not in _TORCH_DT:
        raise VnfError("unsupported tensor dtype %s" % dt)
    return _TORCH_DT[dt]


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

"""ctypes binding of libasr_hip.so (the C ABI declared in include/asr_hip.h).

The library must be built in-tree (``python __graft_entry__.py`` or ``make -C
pytorch_end2end_speech_recognition_amd/csrc``).  There is NO fallback: if the
library is missing or fails to load, every op raises.  torch is imported
first so that the library binds to the HIP runtime torch already loaded
(same soname libamdhip64.so.7).
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the dlopen: shared HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ASR_LIB_PATH: another build of the same library (interleaved A/B runs of two
# kernel versions on one GPU box, tools/gpu_ab.sh); the in-tree build otherwise
LIB_PATH = os.environ.get('ASR_LIB_PATH') or os.path.join(_HERE, 'libasr_hip.so')

c_int = ctypes.c_int
c_ll = ctypes.c_longlong
c_float = ctypes.c_float
c_size = ctypes.c_size_t
c_vp = ctypes.c_void_p
c_str = ctypes.c_char_p

ASR_OK = 0
ASR_ERR_WORKSPACE = -2
ASR_ERR_UNSUPPORTED = -4
ASR_DT_F32 = 0
ASR_DT_BF16 = 1

# name -> (restype, argtypes); must mirror include/asr_hip.h exactly.
SIGNATURES = {
    'asr_version': (c_str, []),
    'asr_last_error': (c_str, []),
    'asr_arch_is_gfx950': (c_int, []),
    'asr_stream_create_cu_masked': (c_int, [c_int, c_int, c_vp]),
    'asr_stream_destroy': (c_int, [c_vp]),
    'asr_ctc_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    'asr_ctc_forward': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int,
                                c_int, c_int, c_vp, c_vp, c_float, c_vp, c_size, c_vp]),
    'asr_ctc_forward_lse': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_vp,
                                    c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_float, c_vp,
                                    c_size, c_vp]),
    'asr_ctc_backward': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int,
                                 c_int, c_vp, c_float, c_vp, c_ll, c_ll, c_vp, c_size, c_vp]),
    'asr_ctc_backward_bf16': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                      c_int, c_int, c_vp, c_float, c_vp, c_ll, c_ll, c_int, c_vp,
                                      c_size, c_vp]),
    'asr_ctc_bias_supported': (c_int, [c_int, c_int, c_int]),
    'asr_ctc_bias_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    'asr_ctc_backward_bf16_db': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                         c_int, c_int, c_vp, c_float, c_vp, c_ll, c_ll, c_int, c_vp,
                                         c_size, c_vp, c_vp, c_size, c_vp]),
    'asr_ctc_fwd_bwd': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int,
                                c_int, c_int, c_vp, c_vp, c_vp, c_size, c_vp]),
    # the four GEMM entry points end in (..., opts: GemmOpts* or NULL)
    'asr_gemm': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'asr_gemm_workspace_bytes': (c_size, [c_vp, c_int, c_vp]),
    'asr_gemm_ws': (c_int, [c_vp, c_int, c_int, c_vp, c_size, c_vp, c_vp]),
    'asr_gemm_lse_ws': (c_int, [c_vp, c_int, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_wgrad_gate': (c_int, [c_vp]),
    'asr_colsum_workspace_bytes': (c_size, [c_int, c_int]),
    'asr_colsum_accumulate': (c_int, [c_vp, c_ll, c_int, c_int, c_float, c_vp, c_vp, c_vp, c_size,
                                      c_vp]),
    'asr_colsum_accumulate_bf16': (c_int, [c_vp, c_ll, c_int, c_int, c_float, c_vp, c_vp, c_vp,
                                           c_size, c_vp]),
    'asr_conv3x3_c1_forward_xs': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                          c_vp, c_int, c_vp]),
    'asr_conv3x3_tr_supported': (c_int, [c_int, c_int, c_int]),
    'asr_conv3x3_tr_plan': (c_int, [c_int, c_int, c_int, c_vp]),
    'asr_conv3x3_tr_has_kernel': (c_int, [c_int, c_int, c_int, c_int]),
    'asr_conv3x3_tr_wgrad_plan': (c_int, [c_int, c_int, c_int, c_vp]),
    'asr_conv3x3_tr': (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_int,
                               c_vp]),
    'asr_vgg_zero_halo': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    'asr_conv3x3_c1_wgrad_workspace_bytes': (c_size, [c_int]),
    'asr_conv3x3_c1_wgrad_xs': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp,
                                        c_vp, c_size, c_vp]),
    'asr_conv3x3_tr_wgrad_workspace_bytes': (c_size, [c_ll, c_int, c_int, c_int]),
    'asr_conv3x3_tr_wgrad': (c_int, [c_vp, c_vp, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_size,
                                     c_vp]),
    'asr_conv3x3_c1_forward': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                       c_vp, c_vp]),
    'asr_lstm_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    # the eight BLSTM layer entry points end in (..., stream, opts: LstmOpts* or NULL)
    'asr_lstm_forward': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp,
                                 c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_backward': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                  c_vp, c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_backward_db': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_backward_dgbf': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                       c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_forward_x': (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                                   c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_forward_x_ok': (c_int, [c_int, c_int, c_int]),
    'asr_lstm_forward_xh': (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                                    c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_forward_xh_drop': (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                         c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_float,
                                         ctypes.c_ulonglong, c_vp, c_size, c_vp, c_vp]),
    'asr_lstm_backward_dgbf_h': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                         c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp, c_vp]),
    'asr_diag_lds_spin': (c_int, [c_int, c_int, c_vp, c_vp]),
    'asr_diag_hold_cus': (c_int, [c_int, c_int, c_int, c_vp]),
    'asr_lstm_unpack_act_h': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_gru_workspace_bytes': (c_size, [c_int, c_int]),
    'asr_gru_forward': (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    'asr_gru_backward': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp,
                                 c_vp, c_size, c_vp]),
    'asr_lstm_uni_shape_ok': (c_int, [c_int, c_int, c_int]),
    'asr_lstm_uni_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    'asr_lstm_uni_forward': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp,
                                     c_vp, c_vp, c_vp, c_size, c_vp]),
    'asr_lstm_uni_backward': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp]),
    'asr_lstm_stream_workspace_bytes': (c_size, [c_int, c_int, c_int]),
    'asr_lstm_stream_forward': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp,
                                        c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp]),
    'asr_ctc_best_path_stream': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_vp,
                                         c_vp, c_vp, c_vp]),
    'asr_gru_cell_forward': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    'asr_gru_cell_backward': (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp,
                                      c_vp]),
    'asr_grad_sqnorm_workspace_bytes': (c_size, []),
    'asr_grad_sqnorm': (c_int, [c_vp, c_ll, c_vp, c_vp, c_size, c_vp]),
    'asr_optim_step': (c_int, [c_int, c_vp, c_vp, c_vp, c_vp, c_ll, c_float, c_float, c_float,
                               c_float, c_float, c_ll, c_float, c_float, c_vp, c_float, c_vp,
                               c_vp]),
    'asr_optim_step_guarded': (c_int, [c_int, c_vp, c_vp, c_vp, c_vp, c_ll, c_float, c_float,
                                       c_float, c_float, c_float, c_ll, c_float, c_float, c_vp,
                                       c_float, c_vp, c_vp, c_vp]),
    'asr_dropout': (c_int, [c_vp, c_vp, c_ll, c_float, ctypes.c_ulonglong, c_vp]),
    'asr_embedding_forward': (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_embedding_backward': (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp,
                                       c_vp]),
    'asr_embedding_backward_csr': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp,
                                           c_vp]),
    'asr_tanh_forward': (c_int, [c_vp, c_vp, c_ll, c_vp]),
    'asr_tanh_backward': (c_int, [c_vp, c_vp, c_vp, c_ll, c_vp]),
    'asr_add_tanh_forward': (c_int, [c_vp, c_vp, c_vp, c_ll, c_vp]),
    'asr_add_forward': (c_int, [c_vp, c_vp, c_vp, c_ll, c_vp]),
    'asr_convert_rows_bf16': None,  # set below, after RowMap (struct passed by value)
    'asr_convert_rows_bf16_dropout': None,
    'asr_ctc_best_path': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp,
                                  c_vp]),
    'asr_row_argmax': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'asr_ctc_beam_ws_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    'asr_ctc_beam_search': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_int,
                                    c_int, c_vp, c_size, c_vp, c_vp, c_vp, c_vp]),
    'asr_ctc_beam_rows': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_int, c_int,
                                  c_vp, c_size, c_vp]),
    'asr_ctc_beam_lm_ws_bytes': (c_size, [c_int] * 7),
    'asr_ctc_beam_search_lm': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_int,
                                       c_int, c_vp, ctypes.c_double, c_vp, c_size, c_vp, c_vp,
                                       c_vp, c_vp]),
    'asr_ctc_beam_stream_state_bytes': (c_size, [c_int] * 7),
    'asr_ctc_beam_stream_ws_bytes': (c_size, [c_int] * 4),
    'asr_ctc_beam_stream_reset': (c_int, [c_vp, c_size, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                          c_vp]),
    'asr_ctc_beam_stream_feed': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_int, c_int,
                                         c_int, c_vp, ctypes.c_double, c_vp, c_vp, c_size, c_int,
                                         c_vp, c_size, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    'asr_ctc_beam_stream_nbest': (c_int, [c_vp, c_size, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    'asr_ctc_beam_stream_status': (c_int, [c_vp, c_int, c_vp, c_vp]),
    'asr_ctc_align_ws_bytes': (c_size, [c_int] * 4),
    'asr_ctc_align': (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int,
                              c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_size, c_vp]),
    'asr_ctc_align_limits': (c_int, [c_vp, c_vp]),
    'asr_edit_distance_ws_bytes': (c_size, [c_int, c_int, c_int]),
    'asr_edit_distance': (c_int, [c_vp, c_ll, c_vp, c_vp, c_ll, c_vp, c_int, c_int, c_int, c_vp,
                                  c_vp, c_vp, c_vp, c_size, c_vp]),
    'asr_xent_workspace_bytes': (c_size, [c_int]),
    'asr_xent_forward': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_float, c_float, c_vp,
                                 c_vp, c_size, c_vp]),
    'asr_xent_backward': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_float, c_float, c_vp,
                                  c_float, c_vp, c_vp, c_size, c_vp]),
    'asr_softmax': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'asr_attdec_workspace_bytes': (c_size, [c_vp, c_int, c_int]),
    'asr_att_trace_read': (c_int, [c_vp]),
    'asr_attdec_chunks': (c_int, [c_vp]),
    'asr_attdec_forward': (c_int, [c_vp, c_int] + [c_vp] * 4 + [c_ll] + [c_vp] * 14 + [c_size,
                                                                                     c_vp]),
    'asr_attdec_backward': (c_int, [c_vp, c_int] + [c_vp] * 4 + [c_ll] + [c_vp] * 19 + [c_size,
                                                                                      c_vp]),
    'asr_attdec_forward_ex': (c_int, [c_vp, c_vp, c_int] + [c_vp] * 4 + [c_ll] + [c_vp] * 14 +
                              [c_size, c_vp]),
    'asr_attdec_backward_ex': (c_int, [c_vp, c_vp, c_int] + [c_vp] * 4 + [c_ll] + [c_vp] * 19 +
                               [c_size, c_vp]),
    'asr_vgg_pad_input': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_conv_weight_pack': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_vgg_pad_input_ch': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_conv_weight_pack_pad': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_conv_weight_unpack_acc_pad': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_conv_weight_unpack_acc_pad_t': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_conv_weight_unpack_acc': (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    'asr_conv_direct_forward': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                        c_vp, c_vp]),
    'asr_conv_direct_dgrad': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                      c_vp]),
    'asr_conv_direct_wgrad_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int, c_int]),
    'asr_conv_direct_wgrad': (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                      c_vp, c_size, c_vp]),
    'asr_vgg_accumulate': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp]),
    'asr_vgg_pool_dims': (c_int, [c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    'asr_vgg_block_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    'asr_vgg_block_forward': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_float, c_float,
                                      c_vp, c_vp, c_float, ctypes.c_ulonglong, c_vp, c_int, c_int,
                                      c_vp, c_size, c_vp]),
    'asr_vgg_block_backward': (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       c_float, ctypes.c_ulonglong, c_vp, c_int, c_vp, c_size,
                                       c_vp]),
    'asr_vgg_block_backward_ex': (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int,
                                          c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_float, ctypes.c_ulonglong, c_vp, c_int, c_vp, c_vp,
                                          c_size, c_vp]),
    'asr_vgg_block_forward_z': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_float,
                                        c_float, c_vp, c_vp, c_float, ctypes.c_ulonglong, c_vp,
                                        c_int, c_int, c_vp, c_size, c_vp]),
    'asr_vgg_block_backward_z': (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_float, ctypes.c_ulonglong, c_vp, c_int, c_vp, c_vp,
                                         c_size, c_vp]),
    'asr_vgg_block_backward_zd': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_float, ctypes.c_ulonglong, c_vp, c_int, c_vp, c_vp,
                                         c_size, c_vp]),
    'asr_vgg_c1_relu_p_blocks': (c_int, [c_int, c_int]),
    'asr_vgg_c1_forward_relu_p': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                          c_vp, c_vp, c_vp, c_vp, c_vp]),
    'asr_vgg_block_forward_given_p': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                              c_vp, c_int, c_float, c_float, c_vp, c_vp, c_float,
                                              ctypes.c_ulonglong, c_vp, c_int, c_int, c_vp, c_vp,
                                              c_int, c_vp, c_size, c_vp]),
    'asr_vgg_block_forward_zp': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                         c_float, c_float, c_vp, c_vp, c_float, ctypes.c_ulonglong,
                                         c_vp, c_int, c_int, c_vp, c_size, c_vp]),
    'asr_vgg_block_backward_zdp': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_int,
                                           c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp,
                                           c_vp, c_vp, c_vp, c_vp, c_float, ctypes.c_ulonglong,
                                           c_vp, c_int, c_vp, c_vp, c_size, c_vp]),
    'asr_conv_taps_supported': (c_int, [c_int] * 8),
    'asr_conv_taps_forward': (c_int, [c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int,
                                      c_int, c_vp, c_vp, c_vp]),
    'asr_conv_taps_dgrad': (c_int, [c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int,
                                    c_int, c_vp, c_vp]),
    'asr_conv_taps_wgrad_workspace_bytes': (c_size, [c_int] * 8),
    'asr_conv_taps_wgrad': (c_int, [c_int, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_vp, c_vp, c_size, c_vp]),
    'asr_conv_taps_weight_pack': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_vp, c_vp]),
    'asr_conv_taps_weight_unpack_acc': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                c_vp]),
    'asr_cnn_act_workspace_bytes': (c_size, [c_int, c_int, c_int, c_int]),
    'asr_cnn_act_forward': (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int,
                                    c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_float,
                                    c_float, c_vp, c_vp, c_float, ctypes.c_ulonglong, c_vp, c_int,
                                    c_int, c_vp, c_size, c_vp]),
    'asr_cnn_act_backward': (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp,
                                     c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                     c_vp, c_vp, c_float, ctypes.c_ulonglong, c_vp, c_int, c_vp,
                                     c_vp, c_vp, c_size, c_vp]),
    'asr_prof_begin': (c_int, [c_int]),
    'asr_prof_end': (c_int, [c_vp, c_vp, c_vp, c_int]),
    'asr_prof_samples': (c_ll, [c_int, c_vp, c_vp, c_vp, c_ll]),
    'asr_lstm_persist_status': (c_int, [c_vp, c_int, c_vp]),
    'asr_lstm_status_gather': (c_int, [c_vp, c_int, c_vp]),
    'asr_lstm_status_inject': (c_int, [c_int, c_vp]),
    'asr_attdec_last_launch': (c_int, [c_vp]),
    'asr_attdec_persist_last': (c_int, [c_vp]),
    'asr_lstm_cell_forward': (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'asr_lstm_cell_backward': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp,
                                       c_vp]),
    'asr_att_step_workspace_bytes': (c_size, [c_vp]),
    'asr_att_step_forward': (c_int, [c_vp] + [c_vp] * 12 + [c_size, c_vp]),
    'asr_att_step_backward': (c_int, [c_vp] + [c_vp] * 21 + [c_size, c_vp]),
    'asr_att_heads_workspace_bytes': (c_size, [c_vp, c_int]),
    'asr_att_heads_forward': (c_int, [c_vp] + [c_vp] * 8 + [c_size, c_vp]),
    'asr_att_heads_backward': (c_int, [c_vp] + [c_vp] * 17 + [c_size, c_vp]),
    'asr_att_beam_ws_bytes': (c_size, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    'asr_att_beam_decode': (c_int, [c_vp, c_vp, c_vp] + [c_vp] * 5 + [c_size] + [c_vp] * 5),
    'asr_lstm_xg_mode': (c_int, [c_vp, c_int]),
    'asr_lstm_last_path': (c_int, [c_vp]),
    'asr_ctc_last_path': (c_int, [c_vp]),
    'asr_ctc_grad_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, c_vp, c_ll, c_ll, c_int, c_int,
                                  c_vp]),
    'asr_ctc_last_lattice_waves': (c_int, []),
    'asr_gemm_last_family': (c_int, []),
    'asr_attdec_conv_feat_bytes': (c_size, [c_vp]),
    'asr_lstm_ws_zero_bytes': (c_size, [c_int, c_int]),
    'asr_lstm_bwd_progress_arrivals': (c_ll, [c_int, c_int, c_int]),
    'asr_lstm_progress_gate': (c_int, [c_vp, c_ll, c_vp]),
    'asr_xg_trace_read': (c_ll, [c_vp]),
    'asr_lstm_debug_dh': (c_int, [c_vp, c_vp, c_vp, c_vp]),
    'asr_lstm_dy_signal': (c_int, [c_vp, c_int, c_int, c_vp]),
    'asr_lstm_backward_grid': (c_int, [c_int, c_int, c_int]),
}


class RowMap(ctypes.Structure):
    """asr_rowmap_t"""
    _fields_ = [('stride_b', c_ll), ('stride_t', c_ll), ('rows_per_b', c_int), ('t_mul', c_int),
                ('t_add', c_int), ('t_limit', c_int), ('perm', c_vp)]


SIGNATURES['asr_convert_rows_bf16'] = (c_int, [c_vp, RowMap, c_int, c_int, c_vp, c_vp])
SIGNATURES['asr_convert_rows_bf16_ld'] = (c_int, [c_vp, RowMap, c_int, c_int, c_int, c_vp, c_vp])
SIGNATURES['asr_convert_rows_bf16_multi'] = (c_int, [c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp])
SIGNATURES['asr_convert_rows_bf16_dropout'] = (c_int, [c_vp, RowMap, c_int, c_int, c_vp, c_float,
                                                        ctypes.c_ulonglong, c_vp])


class Operand(ctypes.Structure):
    """asr_operand_t"""
    _fields_ = [('ptr', c_vp), ('dtype', c_int), ('trans', c_int), ('map', RowMap),
                ('bytes', c_ll), ('tap_group', c_int), ('tap_pitch', c_int), ('tap_sign', c_int)]


class AttDecDims(ctypes.Structure):
    """asr_attdec_dims_t"""
    _fields_ = [(n, c_int) for n in ('B', 'T', 'E', 'A', 'C', 'K', 'D', 'S')] + [
        ('sharpening', c_float), ('sigmoid_smoothing', c_int)]


ATT_HEADS_MAX = 8
ATT_HEADS_MAX_C = 16
ATT_HEADS_ADDITIVE = 0
ATT_HEADS_DOT = 1


class AttHeads(ctypes.Structure):
    """asr_att_heads_t"""
    _fields_ = [(n, c_int) for n in ('B', 'T', 'E', 'A', 'C', 'K', 'D', 'H', 'kind')] + [
        ('sharpening', c_float), ('sigmoid_smoothing', c_int)] + [
        (n, c_vp * ATT_HEADS_MAX) for n in ('w_dec', 'w_conv', 'conv_w', 'v')]


class AttDecOpts(ctypes.Structure):
    """asr_attdec_opts_t (decoder dropout + scheduled sampling + kept conv features)"""
    _fields_ = [('dropout_hidden', c_float), ('seed_hidden', ctypes.c_ulonglong),
                ('ss_steps_host', c_vp), ('Y', c_int), ('Dz', c_int), ('V', c_int),
                ('w_d', c_vp), ('b_d', c_vp), ('drop_d', c_float), ('seed_d', ctypes.c_ulonglong),
                ('w_c', c_vp), ('b_c', c_vp), ('drop_c', c_float), ('seed_c', ctypes.c_ulonglong),
                ('w_fc', c_vp), ('b_fc', c_vp), ('emb_w', c_vp), ('emb_trans', c_int),
                ('drop_emb', c_float), ('seed_emb', ctypes.c_ulonglong), ('w_ih_emb', c_vp),
                ('ld_ih', c_ll), ('b_ih', c_vp), ('b_hh', c_vp), ('pre_ss', c_vp),
                ('emb_ss', c_vp), ('tok_ss', c_vp), ('d_pre', c_vp), ('dg_ss', c_vp),
                ('conv_feat', c_vp)]


class LstmOpts(ctypes.Structure):
    """asr_lstm_opts_t (one recurrence call's launch settings; all zero: the defaults)"""
    _fields_ = [('ws_prezeroed', c_int), ('bwd_pin_kb', c_int), ('bwd_units', c_int),
                ('dy_flags', c_vp), ('dy_c0', c_int), ('dy_epoch', c_int), ('progress', c_vp),
                ('progress_q1', c_int), ('progress_q2', c_int)]


class GemmOpts(ctypes.Structure):
    """asr_gemm_opts_t (one GEMM call's settings; all zero: the defaults)"""
    _fields_ = [('small_tiles', c_int), ('nosplit', c_int), ('n64_kmode', c_int)]


class CtcGradPlan(ctypes.Structure):
    """asr_ctc_grad_plan_t"""
    _fields_ = [(n, c_int) for n in ('path', 'nch', 'aligned', 'threads', 'rpb', 'nblk', 'rev',
                                     'acts_bytes')] + [('lds_bytes', c_size), ('part_bytes', c_size)]


def ctc_grad_plan(T, B, V, gld, max_label_len, acts_addr, stride_t, stride_b, with_bias, cus=0):
    """asr_ctc_grad_plan: the gradient pass's plan for these shapes (host only;
    cus = 0 asks the current device).  Raises NativeError where the pass refuses."""
    plan = CtcGradPlan()
    call('asr_ctc_grad_plan', T, B, V, gld, max_label_len, ctypes.c_void_p(acts_addr), stride_t,
         stride_b, int(bool(with_bias)), cus, ctypes.byref(plan))
    return plan


def conv3x3_tr_plan(cin, cout, fp):
    """asr_conv3x3_tr_plan: (wpx, nw, RC, LDS bytes) of the tap-resident
    convolution at this channel pair and row pitch (host only), or None where
    the kernel does not take the shape."""
    out = (c_int * 4)()
    if not query('asr_conv3x3_tr_plan', int(cin), int(cout), int(fp), out):
        return None
    return tuple(out)


def conv3x3_tr_wgrad_plan(cin, cout, fp):
    """asr_conv3x3_tr_wgrad_plan: (RC, LDS bytes) of the tap-resident weight
    gradient (host only), or None where the kernel does not take the shape."""
    out = (c_int * 2)()
    if not query('asr_conv3x3_tr_wgrad_plan', int(cin), int(cout), int(fp), out):
        return None
    return tuple(out)


class AttBeamOpts(ctypes.Structure):
    """asr_att_beam_opts_t"""
    _fields_ = [(n, c_int) for n in ('W', 'V', 'Y', 'Dz', 'max_len', 'min_len', 'eos',
                                     'emb_trans')] + [
        ('length_penalty', ctypes.c_double), ('ld_ih', c_ll)] + [
        (n, c_vp) for n in ('w_ih', 'w_hh', 'b_ih', 'b_hh', 'w_dec', 'w_conv', 'conv_w', 'v',
                            'w_d', 'b_d', 'w_c', 'b_c', 'w_fc', 'b_fc', 'emb_w')]


class AttBeamCtc(ctypes.Structure):
    """asr_att_beam_ctc_t"""
    _fields_ = [('ctc_logits', c_vp), ('Vc', c_int), ('blank', c_int), ('label_offset', c_int),
                ('weight', ctypes.c_double)]


ATT_BEAM_CELL_LSTM = 0
ATT_BEAM_CELL_GRU = 1


class AttBeamEx(ctypes.Structure):
    """asr_att_beam_ex_t"""
    _fields_ = [('cell', c_int), ('ctc', c_vp), ('lm', c_vp)]


ATT_BEAM_LM_MAX_LAYERS = 4


class AttBeamLm(ctypes.Structure):
    """asr_att_beam_lm_t"""
    _fields_ = [(n, c_int) for n in ('layers', 'H', 'Y', 'V', 'cell')] + [('emb', c_vp)] + [
        (n, c_vp * ATT_BEAM_LM_MAX_LAYERS) for n in ('w_ih', 'w_hh', 'b_ih', 'b_hh')] + [
        ('w_out', c_vp), ('b_out', c_vp), ('weight', ctypes.c_double)]


ASR_ED_TOKEN = 0
ASR_ED_WORD = 1


class EditOpts(ctypes.Structure):
    """asr_edit_opts_t"""
    _fields_ = [('unit', c_int), ('eos', c_int), ('space', c_int), ('map', c_vp),
                ('map_len', c_int), ('hyp_i64', c_int)]


class Gemm(ctypes.Structure):
    """asr_gemm_t"""
    _fields_ = [('a', Operand), ('b', Operand), ('c', c_vp), ('c_map', RowMap), ('bias', c_vp),
                ('bias2', c_vp), ('M', c_int), ('N', c_int), ('K', c_int), ('alpha', c_float),
                ('beta', c_float), ('batch', c_int), ('batch_stride_a', c_ll),
                ('batch_stride_b', c_ll), ('batch_stride_c', c_ll), ('drop_p', c_float),
                ('drop_seed', ctypes.c_ulonglong), ('c_dtype', c_int)]


class NativeError(RuntimeError):
    """Raised for any failure of the native library (load or call).  A
    RuntimeError, so the reference's train_step skip-batch policy
    (utils/training/training_loop.py:69-76) applies unchanged."""


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError('libasr_hip.so not built at %s -- run `python -c "import '
                              '__graft_entry__ as g; g.build()"` (no CPU fallback exists)'
                              % LIB_PATH)
        try:
            h = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            raise NativeError('failed to load %s: %s' % (LIB_PATH, e))
        ab = bool(os.environ.get('ASR_LIB_PATH'))
        for name, (res, args) in SIGNATURES.items():
            if ab and not hasattr(h, name):
                continue   # an older A/B build without this entry point
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != ASR_OK:
        msg = lib().asr_last_error().decode(errors='replace')
        raise NativeError('%s failed (rc=%d): %s' % (name, rc, msg))
    return rc


def query(name, *args):
    return getattr(lib(), name)(*args)


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def ptr_struct(s):
    """Pointer to a ctypes struct (None -> NULL)."""
    return None if s is None else ctypes.byref(s)


def stream_handle(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_arch_ok = []


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError('HIP op called with a CPU tensor (no CPU fallback by design)')
    if not _arch_ok:
        # the code objects are gfx950 only: say so instead of failing to launch
        a = lib().asr_arch_is_gfx950()
        if a != 1:
            raise NativeError('libasr_hip.so is built for gfx950 (MI355X) only; the current '
                              'device is not one (asr_arch_is_gfx950 = %d)' % a)
        _arch_ok.append(True)

"""Thin tensor-level wrappers over the C ABI (include/seld_hip.h) + the autograd glue, one module per kernel family;
`_core` holds what they share.  Every name is reached as `hip_ops.<name>`.

Everything here requires CUDA(HIP) tensors: fp32, contiguous.  No eager/CPU fallback exists.
"""
from ._core import *            # noqa: F401,F403
from .train_ops import *        # noqa: F401,F403
from .norm_act import *         # noqa: F401,F403
from .conv3d import *           # noqa: F401,F403
from .weight_forms import *     # noqa: F401,F403
from .streams import *          # noqa: F401,F403
from .conv import *             # noqa: F401,F403
from .conv_transpose import *   # noqa: F401,F403
from .dwconv import *           # noqa: F401,F403
from .linear_mha import *       # noqa: F401,F403
from .first_stage import *      # noqa: F401,F403
from .quat import *             # noqa: F401,F403
from .labels import *           # noqa: F401,F403
from .loader import *           # noqa: F401,F403
from .event_metrics import *    # noqa: F401,F403
from .ensemble import *         # noqa: F401,F403
from .smooth import *           # noqa: F401,F403
from .squeeze_excite import *   # noqa: F401,F403
from .temporal_attention import *  # noqa: F401,F403
from .features import *         # noqa: F401,F403
from .gru import *              # noqa: F401,F403
# `import *` skips underscore names: the ones the training harness, the tests and tools/ reach, and the rest of the module surface
from ._core import _drop_kernel_choice_caches, _pair, _req, _scratch_pools  # noqa: F401
from .train_ops import _req_inplace, _unit_gradients  # noqa: F401
from .norm_act import (_claim_grad_slots, _direct_targets, _identity_cache, _nbt, _ncs, _one_pass_ok, _Philox,  # noqa: F401
                       _rowscale, _stats_pool)
from .conv3d import _conv3d_backward, _conv3d_weights, _triple  # noqa: F401
from .weight_forms import _GruWeights, _hcq_ok, _HcqWeights  # noqa: F401
from .streams import _on_side_stream, _side_enabled  # noqa: F401
from .conv import (_conv_backward, _DeferredWgrads, _hcq_wgrad_label, _hcq_wgrad_ok, _label,  # noqa: F401
                   _pair_ok, _ptr2, _transpose_ahead, _y_shape)
from .dwconv import _dw_y_shape  # noqa: F401
from .linear_mha import _mha_keep_mask  # noqa: F401
from .first_stage import _first_stage_nostore, _fs_bytes  # noqa: F401
from .quat import (_quat_cat1_shape, _quat_modulus_sum, _quat_summed_shape, _quat_ws, _QuatUnaryFn, _rot_check,  # noqa: F401
                   _rot_dims)
from .features import _band_tables, _feature_form, _features_of_planes, _mel_tables  # noqa: F401

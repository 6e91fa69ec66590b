"""transmf_ad_amd — MI355X-native (gfx950) forward/backward hot path of TransMF_AD.

    from transmf_ad_amd import model_ad, model_CNN_ad, model_single
    from transmf_ad_amd import model_CNN, model_transformer, model_transformer_res

are drop-ins for the reference's ``models.mymodel`` classes (same constructors, forward
signatures, state_dict keys).  All hot-path compute runs in hand-written HIP kernels behind the
C ABI of ``include/tmf_hip.h`` (``libtmf_hip.so``, built by ``python -m transmf_ad_amd.build``);
there is no CPU / stock-PyTorch fallback.
"""
from ._lib import LIB_PATH, TmfError, load as load_library          # noqa: F401
from .gradient_reversal import GradientReversal, revgrad            # noqa: F401
from .mymodel import (model_ad, model_CNN, model_CNN_ad, model_single, model_transformer,   # noqa: F401
                      model_transformer_res)
from .ops import get_conv_precision, set_activation_storage, set_conv_precision   # noqa: F401
from .pipeline import DeviceDataset, DevicePrefetcher, scale_intensity_flip, rotate_zoom   # noqa: F401
from .nifti import read_nifti, write_nifti, nifti_batches         # noqa: F401
from . import optim                                                  # noqa: F401
from .losses import FALoss, SupConLoss                               # noqa: F401
from .saliency import input_gradients, integrated_gradients        # noqa: F401
from .attention_maps import attention_maps, attention_maps_torch   # noqa: F401
from .gradcam import grad_cam, grad_cam_torch                      # noqa: F401
from .occlusion import occlusion_sensitivity, occlusion_sensitivity_torch   # noqa: F401
from .faithfulness import faithfulness_curve, faithfulness_curve_torch   # noqa: F401
from .region_stats import RegionAccumulator, RegionStats, region_stats, region_stats_torch   # noqa: F401
from .clusters import Clusters, clusters, clusters_torch       # noqa: F401
from .smooth import gaussian_smooth, gaussian_smooth_torch     # noqa: F401
from .rise import Rise, rise, rise_torch                       # noqa: F401
from .region_shap import RegionShap, region_shap, region_shap_torch   # noqa: F401
from .networks import (Attention, CrossTransformer, CrossTransformer_MOD_AVG, FeedForward, PreNorm,   # noqa: F401
                       Transformer, sNet)

__all__ = ["model_ad", "model_CNN_ad", "model_single", "model_CNN", "model_transformer", "model_transformer_res", "sNet",
           "CrossTransformer", "CrossTransformer_MOD_AVG", "Transformer",
           "Attention", "PreNorm", "FeedForward", "revgrad", "GradientReversal", "load_library", "TmfError",
           "set_conv_precision", "get_conv_precision", "set_activation_storage", "DeviceDataset", "DevicePrefetcher", "scale_intensity_flip", "rotate_zoom",
           "read_nifti", "write_nifti", "nifti_batches", "FALoss", "SupConLoss",
           "input_gradients", "integrated_gradients", "attention_maps", "attention_maps_torch",
           "grad_cam", "grad_cam_torch", "occlusion_sensitivity", "occlusion_sensitivity_torch",
           "faithfulness_curve", "faithfulness_curve_torch",
           "region_stats", "region_stats_torch", "RegionStats", "RegionAccumulator",
           "clusters", "clusters_torch", "Clusters", "gaussian_smooth", "gaussian_smooth_torch",
           "rise", "rise_torch", "Rise", "region_shap", "region_shap_torch", "RegionShap"]

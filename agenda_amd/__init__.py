"""agenda_amd -- MI355X-native (gfx950) implementation of the AGenDA data-generation hot path:
Stable-Diffusion UNet denoise loop + DAAM cross-attention heat maps + VAE decode, as hand-written
HIP kernels behind a C ABI (include/agenda_hip.h), with the Python call surfaces the reference
scripts use (StableDiffusionPipeline, daam.trace, the attention-processor hooker)."""
from . import config, synthetic, ip_adapter  # noqa: F401
from .pipeline import StableDiffusionPipeline, PipelineOutput, Engine, DeepCacheSDHelper  # noqa: F401
from .pipeline import StableDiffusionPipeline as StableDiffusionPAGPipeline  # noqa: F401  (diffusers' name: the same class, pag_applied_layers=)
from .pipeline import StableDiffusionPipeline as SemanticStableDiffusionPipeline  # noqa: F401  (diffusers' name: the same class, editing_prompt=)
from .trace import trace, GlobalHeatMap, WordHeatMap, compute_token_merge_indices  # noqa: F401
from .hook import UNetCrossAttentionHooker  # noqa: F401
from .scheduler import DDIMScheduler  # noqa: F401
from .controlnet import ControlNetModel, StableDiffusionControlNetPipeline  # noqa: F401
from .adapter import T2IAdapter, StableDiffusionAdapterPipeline  # noqa: F401
from .inpaint import StableDiffusionInpaintPipeline  # noqa: F401
from .ip2p import StableDiffusionInstructPix2PixPipeline  # noqa: F401
from .gligen import StableDiffusionGLIGENPipeline  # noqa: F401
from .panorama import StableDiffusionPanoramaPipeline, get_views  # noqa: F401
from .regions import StableDiffusionRegionPipeline  # noqa: F401

__all__ = ["StableDiffusionPipeline", "StableDiffusionPAGPipeline", "SemanticStableDiffusionPipeline", "PipelineOutput", "Engine", "trace", "GlobalHeatMap", "WordHeatMap",
           "compute_token_merge_indices", "UNetCrossAttentionHooker", "DDIMScheduler", "config", "synthetic", "ip_adapter",
           "ControlNetModel", "StableDiffusionControlNetPipeline", "T2IAdapter", "StableDiffusionAdapterPipeline",
           "StableDiffusionInpaintPipeline",
           "StableDiffusionInstructPix2PixPipeline",
           "StableDiffusionGLIGENPipeline", "StableDiffusionPanoramaPipeline", "get_views", "StableDiffusionRegionPipeline", "DeepCacheSDHelper"]

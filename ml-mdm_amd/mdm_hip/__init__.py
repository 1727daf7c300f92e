"""mdm_hip -- MI355X-native (gfx950) U-Net / NestedUNet denoiser hot path for ml-mdm.

Layout of the package
  _lib.py         build + ctypes binding of libmdm_hip.so (C ABI in include/mdm_hip.h)
  ops.py          torch.autograd tape entries around the C ABI
  unet.py         UNet, config dataclasses (mirror of ml_mdm.models.unet)
  nested_unet.py  NestedUNet (mirror of ml_mdm.models.nested_unet)
  diffusion.py    Diffusion / NestedDiffusion train-step + sampling call surface; invert / sample_from / Inverted: image
                  inversion (DDIM fixed point, DDPM noise maps: samplers.Sampler.invert / noise_maps / step_noise=)
  samplers.py     noise schedules + DDPM/DDIM updates, DPM-Solver++(2M), SASolver (SA-Solver: predictor-corrector); LossGuide: loss-guided (DPS) sampling through the model's input gradient;
                  SampleOptions: the sampling options beyond the reference, their checks and what they compose with
  configs.py      the three shipped architectures (cc12m 64 / 256 / 1024)
  distributed.py  one-process-per-GPU data parallel gradient reducer over RCCL
  registry.py     plug into the reference's ml_mdm.config registries when present
  text_encoder.py T5Encoder / LanguageModel: the frozen flan-T5 text encoder on packed tokens (mirror of
                  ml_mdm.language_models.factory)
  lora.py         LoRA adapters on the attention projections: attach / merge / unmerge / detach
  textual_inversion.py  learnable placeholder-token embeddings through the frozen text encoder: attach / merge / detach
  fp8.py          opt-in MXFP8 (weights and activations) sampling path of the attention-layer 1x1 GEMMs and, with
                  conv_targets, of the ResNet convolutions (3x3 implicit GEMM): attach / detach
  pag.py          perturbed-attention guidance: select / perturbed (the samplers' pag_scale / pag_layers)
  regions.py      regional prompts and token weights, a bias on the text cross-attention logits: RegionPrompts / concat /
                  applied (the samplers' regions / region_layers)
  attn_control.py prompt-to-prompt attention control, an edited batch row computing with its source row's attention maps:
                  AttnControl / applied (the samplers' control)
  attn_maps.py    cross-attention maps, the text term's probabilities recorded per token: AttnMaps / record / applied (the
                  samplers' attn_maps); GradRows / cross_probs: the maps on the autograd tape, for the samplers' map_guide
                  (samplers.MapGuide, samplers.AttendExcite: attention-map guidance, Attend-and-Excite)
  freeu.py        FreeU on the up path's skip concat: FreeU / select / applied (the samplers' freeu)
  guidance.py     projected and rescaled classifier-free guidance (APG, CFG rescale, guidance interval): CFG / cfg_combine
                  (the samplers' cfg)
  tiling.py       tiled (MultiDiffusion) sampling of canvases larger than the model's window: Tiles / gather / merge (the
                  samplers' tiles)
"""
import os as _os

# ROCclr maps a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and a queue is in order: with more
# streams than queues -- the data-parallel step has six: main, weight-gradient, communication, completion, RCCL's own, the
# null stream -- kernels of one stream wait behind barrier packets (or collectives) of another.  Measured with every bucket
# forced through RCCL in a world of one: +2.65 -> +1.6 ms per step under 8 queues, the plain step unchanged
# (profiles/r06_did_not_pay.md).  Read when the HIP runtime initialises (the first HIP call of the process), so this
# has to happen before any; an explicit setting in the environment wins.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from . import _lib  # noqa: F401,E402
from .nested_unet import (  # noqa: E402  # noqa: F401
    Nested2UNetConfig,
    Nested3UNetConfig,
    Nested4UNetConfig,
    NestedUNet,
    NestedUNetConfig,
)
from .text_encoder import LanguageModel, T5Encoder, T5EncoderConfig  # noqa: F401,E402
from .unet import ResNetConfig, UNet, UNetConfig  # noqa: F401,E402
from . import lora  # noqa: F401,E402
from . import fp8  # noqa: F401,E402
from .ops import activation_recompute_enabled, enable_activation_recompute  # noqa: F401,E402
from .samplers import AttendExcite, LossGuide, MapGuide, SASolver  # noqa: F401,E402
from .diffusion import Inverted  # noqa: F401,E402
from . import pag  # noqa: F401,E402
from . import regions  # noqa: F401,E402
from .regions import RegionPrompts  # noqa: F401,E402
from . import attn_maps  # noqa: F401,E402
from .attn_maps import AttnMaps  # noqa: F401,E402
from . import attn_control  # noqa: F401,E402
from .attn_control import AttnControl  # noqa: F401,E402
from . import freeu  # noqa: F401,E402
from .freeu import FreeU  # noqa: F401,E402
from . import guidance  # noqa: F401,E402
from .guidance import CFG  # noqa: F401,E402
from . import tiling  # noqa: F401,E402
from .tiling import Tiles  # noqa: F401,E402
from . import textual_inversion  # noqa: F401,E402

__all__ = [
    "textual_inversion",
    "tiling",
    "Tiles",
    "guidance",
    "CFG",
    "freeu",
    "FreeU",
    "pag",
    "regions",
    "RegionPrompts",
    "attn_maps",
    "AttnMaps",
    "attn_control",
    "AttnControl",
    "UNet",
    "UNetConfig",
    "ResNetConfig",
    "NestedUNet",
    "NestedUNetConfig",
    "Nested2UNetConfig",
    "Nested3UNetConfig",
    "Nested4UNetConfig",
    "T5Encoder",
    "T5EncoderConfig",
    "LanguageModel",
    "lora",
    "fp8",
    "enable_activation_recompute",
    "activation_recompute_enabled",
    "LossGuide",
    "MapGuide",
    "AttendExcite",
    "SASolver",
    "Inverted",
]

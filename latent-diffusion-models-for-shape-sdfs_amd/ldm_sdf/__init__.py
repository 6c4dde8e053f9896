"""ldm_sdf -- MI355X-native hot path of latent diffusion over DeepSDF shape codes.

Layers: ``api`` (train/sample/decode) -> ``models`` (parameter containers,
packing) -> ``ops`` (one wrapper per C-ABI call) -> ``_capi`` (ctypes) -> ``libldm_sdf.so``
(HIP kernels for gfx950, sources in ``../csrc``).  ``dist`` adds z-slab / batch sharding
over ``torch.distributed`` (RCCL).
"""
from .models import DDPMSchedule, MLPDenoiser, SDFDecoder, decoder_layer_dims  # noqa: F401
from .unet import UNet1DDenoiser  # noqa: F401
from .mesh import (marching_cubes, marching_cubes_batch, mc_table, vertex_normals,  # noqa: F401
                   write_ply, read_ply, read_obj)
from .api import (Sampler, TrainState, decode, decode_points, resolve_decode_dtype,  # noqa: F401
                  sample, train, train_step)
from .band import (BandInfo, decode_band, extract_mesh, lattice_indices,  # noqa: F401
                   n_bricks)
from .autodecoder import (AutoDecoderState, autodecoder_train_step,  # noqa: F401
                          train_autodecoder)
from .grad import fit_latents, sdf_grad  # noqa: F401
from .meshsdf import mesh_sdf, normalize_mesh, sample_sdf, sample_surface  # noqa: F401
from .metrics import (chamfer_distance, chamfer_matrix, emd_distance,  # noqa: F401
                      emd_matrix, evaluate_generation, generation_metrics, nearest_points,
                      shape_clouds)
from .render import (camera_rays, depth_samples, estimate_lipschitz, look_at,  # noqa: F401
                     ray_mesh, read_png, render_mesh, render_sdf, trace_sdf, write_png)
from . import ops, dist, pack, data, meshsdf, metrics, render  # noqa: F401
from ._capi import LdmError, load as load_library  # noqa: F401

__version__ = "0.1.0"

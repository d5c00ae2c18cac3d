"""`frido.models.diffusion.dpm_solver` import path (where upstream latent-diffusion keeps its DPMSolverSampler) -> HIP-backed sampler."""
from frido_amd.samplers import DPMSolverSampler  # noqa: F401

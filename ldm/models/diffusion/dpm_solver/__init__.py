from .sampler import DPMSolverSampler

__all__ = ["DPMSolverSampler"]

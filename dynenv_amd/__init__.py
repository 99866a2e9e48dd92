"""dynenv_amd — MI355X-native batched step() for DynEnv (drop-in for the reference's make_dyn_env path).

Only what the hot path needs lives here: csrc/ (HIP kernels + the C ABI of include/dynenv.h) and the host-side
mirror of the reference's vectorised-environment interface.
"""
from .enums import DynEnvType, NoiseType, ObservationType
from .vec_env import BatchedDynEnv, make_dyn_env
from .arranger import GpuInOutArranger, groups_for

__all__ = ["BatchedDynEnv", "make_dyn_env", "DynEnvType", "NoiseType", "ObservationType", "GpuInOutArranger", "GpuInputLayer",
           "GpuEmbedInputLayer", "EmbedBlock", "GpuTemporalAttention", "GpuRecurrentHead", "GpuFeatureExtractor", "GpuPolicyHead", "GpuRolloutStorage", "GpuRollout", "GpuICM", "groups_for"]


def __getattr__(name):
    if name in ("GpuInputLayer", "GpuEmbedInputLayer", "EmbedBlock"):   # nn.Modules: built on first use, so that the package imports without torch
        from . import arranger
        return getattr(arranger, name)
    if name == "GpuTemporalAttention":
        from . import attention
        return attention.GpuTemporalAttention
    if name in ("GpuRecurrentHead", "GpuFeatureExtractor"):
        from . import recurrent
        return getattr(recurrent, name)
    if name == "GpuPolicyHead":
        from . import policy
        return policy.GpuPolicyHead
    if name in ("GpuRolloutStorage", "GpuRollout"):
        from . import rollout
        return getattr(rollout, name)
    if name == "GpuICM":
        from . import icm
        return icm.GpuICM
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

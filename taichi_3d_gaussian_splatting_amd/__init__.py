"""MI355X-native rasterisation operator, drop-in for the hot path of
Wenri/taichi_3d_gaussian_splatting.  Importing the package does not
load the HIP library; constructing the operator does, and fails loudly without it."""
from .Camera import CameraInfo  # noqa: F401
from .GaussianPointCloudRasterisation import GaussianPointCloudRasterisation  # noqa: F401
from .controller_stats import ControllerAccumulators  # noqa: F401
from .GaussianPointAdaptiveController import GaussianPointAdaptiveController  # noqa: F401
from .GaussianPointCloudScene import GaussianPointCloudScene  # noqa: F401
from .LossFunction import LossFunction  # noqa: F401
from .ImagePoseDataset import ImagePoseDataset  # noqa: F401
from .targets import TargetStore, image_resample  # noqa: F401
from .GaussianPointTrainer import GaussianPointCloudTrainer  # noqa: F401
from . import mixture  # noqa: F401
from . import compose, frames, fusion  # noqa: F401
from .GaussianPointRenderer import GaussianPointRenderer  # noqa: F401

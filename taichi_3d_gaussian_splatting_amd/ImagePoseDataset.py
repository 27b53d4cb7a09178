"""ImagePoseDataset -- the reference's dataset (taichi_3d_gaussian_splatting/ImagePoseDataset.py) without torchvision:
the same JSON (pandas, orient="records"), the same item (image (3,H,W) f32 on the CPU, q (1,4), t (1,3), CameraInfo), the
intrinsics rescaled to the real image size, the crop to multiples of 16 and the autoscale of images over 1600 pixels.
to_tensor is uint8 / 255 and the antialiased resize is F.interpolate(mode="bilinear", antialias=True): the operator
torchvision's resize calls.  load_raw() is the decoded image before any of that, for targets.TargetStore."""
import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data

from .Camera import CameraInfo
from .targets import MAX_RESOLUTION_TRAIN, autoscaled_camera_info  # noqa: F401
from .utils import SE3_to_quaternion_and_translation_torch

TILE_WIDTH = TILE_HEIGHT = 16


def resize_antialias(image: torch.Tensor, size) -> torch.Tensor:
    """torchvision.transforms.functional.resize(image, size=(h, w), antialias=True) of a float (C,H,W) tensor"""
    return F.interpolate(image.unsqueeze(0), size=(int(size[0]), int(size[1])), mode="bilinear", antialias=True,
                         align_corners=False).squeeze(0)


REQUIRED_COLUMNS = ("image_path", "T_pointcloud_camera", "camera_intrinsics", "camera_height", "camera_width", "camera_id")


def _f32(field) -> torch.Tensor:
    """a JSON field (nested lists, an array or a tensor) as a float32 tensor of its own"""
    if isinstance(field, torch.Tensor):
        return field.to(torch.float32).clone()
    return torch.from_numpy(np.array(field, dtype=np.float32))


class ImagePoseDataset(torch.utils.data.Dataset):
    """Images, poses and camera intrinsics of one dataset JSON: a list of records with REQUIRED_COLUMNS."""

    def __init__(self, dataset_json_path: str):
        super().__init__()
        import pandas as pd         # here and not at the top: importing the package needs neither pandas nor PIL
        self.df = pd.read_json(dataset_json_path, orient="records")
        missing = [c for c in REQUIRED_COLUMNS if c not in self.df.columns]
        assert not missing, f"column {missing[0]} is not in the dataset"

    def __len__(self):
        return len(self.df)

    @staticmethod
    def _autoscale_image_and_camera_info(image: torch.Tensor, camera_info: CameraInfo):
        """an image over MAX_RESOLUTION_TRAIN on either side: resize(size=1024, max_size=1600, antialias=True), the crop to
        multiples of 16 and the intrinsics scaled with it (ImagePoseDataset.py:41-62); anything else passes unchanged"""
        size_full, resized_info = autoscaled_camera_info(camera_info)
        if size_full is None:
            return image, camera_info
        image = resize_antialias(image, size_full)
        return image[:3, :resized_info.camera_height, :resized_info.camera_width].contiguous(), resized_info

    def load_raw(self, idx):
        """-> (image uint8 (H,W,3|4) CPU tensor as decoded, uncropped; q (1,4); t (1,3); CameraInfo of the cropped image:
        intrinsics rescaled to the real image size, height and width cut to multiples of 16, before any autoscale)"""
        import PIL.Image
        row = self.df.iloc[idx]
        q, t = SE3_to_quaternion_and_translation_torch(_f32(row["T_pointcloud_camera"]).unsqueeze(0))
        with PIL.Image.open(row["image_path"]) as pil:
            image = torch.from_numpy(np.array(pil if pil.mode in ("RGB", "RGBA") else pil.convert("RGB"), dtype=np.uint8))
        height, width = image.shape[0], image.shape[1]
        # the JSON's size is COLMAP's; the intrinsics follow the size the file really has
        k = _f32(row["camera_intrinsics"])
        k[0, :] = k[0, :] * width / row["camera_width"]
        k[1, :] = k[1, :] * height / row["camera_height"]
        info = CameraInfo(camera_intrinsics=k, camera_height=height - height % TILE_HEIGHT, camera_width=width - width % TILE_WIDTH,
                          camera_id=row["camera_id"])
        return image, q, t, info

    def load_mask(self, idx):
        """-> the mask of record idx as a uint8 (H,W) array, 255 = use and 0 = ignore, or None when the dataset has no
        mask_path column or the record's entry is empty.  The file is an 8-bit single-channel image of the picture's size
        (anything else is converted to 8-bit grey)."""
        if "mask_path" not in self.df.columns:
            return None
        path = self.df.iloc[idx]["mask_path"]
        if not isinstance(path, str) or not path:
            return None
        import PIL.Image
        with PIL.Image.open(path) as pil:
            return np.array(pil if pil.mode == "L" else pil.convert("L"), dtype=np.uint8)

    def load_depth(self, idx):
        """-> (depth map, depth_scale) of record idx, or None when the dataset has no depth_path column or the record's entry is
        empty.  depth_path names a 16-bit single-channel PNG (-> a uint16 (H,W) array, 0 = no measurement) or a .npy of float32
        metres (-> a float32 (H,W) array; anything not finite and > 0 = no measurement).  depth_scale: the record's depth_scale
        column, metres per unit of the 16-bit file, or None (the caller's default applies).  The map must have the decoded
        picture's size, and the picture must be within MAX_RESOLUTION_TRAIN: there is no autoscale path for depth."""
        if "depth_path" not in self.df.columns:
            return None
        row = self.df.iloc[idx]
        path = row["depth_path"]
        if not isinstance(path, str) or not path:
            return None
        import PIL.Image
        with PIL.Image.open(row["image_path"]) as pil:
            width, height = pil.size                            # the header only: nothing is decoded
        if height > MAX_RESOLUTION_TRAIN or width > MAX_RESOLUTION_TRAIN:
            raise ValueError(f"{path}: depth for a picture over {MAX_RESOLUTION_TRAIN} pixels ({width}x{height}) is not supported "
                             "(there is no autoscale path for depth)")
        if path.lower().endswith(".npy"):
            depth = np.load(path)
            if depth.ndim != 2 or depth.dtype.kind != "f":
                raise ValueError(f"{path}: a .npy depth map must be a 2-D float array, got {depth.dtype} {depth.shape}")
            depth = depth.astype(np.float32, copy=False)
        else:
            with PIL.Image.open(path) as pil:
                if pil.mode not in ("I;16", "I;16L", "I;16B", "I"):
                    raise ValueError(f"{path}: a depth image must be a 16-bit single-channel PNG, got mode {pil.mode}")
                depth = np.array(pil)
            if depth.ndim != 2 or depth.min() < 0 or depth.max() > 65535:
                raise ValueError(f"{path}: a depth image must hold 16-bit values")
            depth = depth.astype(np.uint16)
        if depth.shape != (height, width):
            raise ValueError(f"{path}: the depth map is {depth.shape[1]}x{depth.shape[0]}, the picture {width}x{height}")
        scale = None
        if "depth_scale" in self.df.columns:
            value = row["depth_scale"]
            if value is not None and not (isinstance(value, float) and np.isnan(value)):
                scale = float(value)
        return depth, scale

    def load_normal(self, idx):
        """-> the normal prior of record idx, or None when the dataset has no normal_path column or the record's entry is
        empty.  normal_path names an 8-bit RGB image that holds (n + 1) / 2 (-> a uint8 (H,W,3) array; (0,0,0) = no prior) or
        a .npy of float32 (H,W,3) normals (-> a float32 (H,W,3) array; all zero or not finite = no prior).  Which camera frame the
        normals are in is the caller's to say (geometry.normal_flags).  The map must have the decoded picture's size, and the
        picture must be within MAX_RESOLUTION_TRAIN: there is no autoscale path for normals."""
        if "normal_path" not in self.df.columns:
            return None
        row = self.df.iloc[idx]
        path = row["normal_path"]
        if not isinstance(path, str) or not path:
            return None
        import PIL.Image
        with PIL.Image.open(row["image_path"]) as pil:
            width, height = pil.size                            # the header only: nothing is decoded
        if height > MAX_RESOLUTION_TRAIN or width > MAX_RESOLUTION_TRAIN:
            raise ValueError(f"{path}: normals for a picture over {MAX_RESOLUTION_TRAIN} pixels ({width}x{height}) are not supported "
                             "(there is no autoscale path for normals)")
        if path.lower().endswith(".npy"):
            normal = np.load(path)
            if normal.ndim != 3 or normal.shape[2] != 3 or normal.dtype.kind != "f":
                raise ValueError(f"{path}: a .npy normal map must be a float (H,W,3) array, got {normal.dtype} {normal.shape}")
            normal = normal.astype(np.float32, copy=False)
        else:
            with PIL.Image.open(path) as pil:
                if pil.mode not in ("RGB", "RGBA"):
                    raise ValueError(f"{path}: a normal image must be an 8-bit RGB image, got mode {pil.mode}")
                normal = np.array(pil, dtype=np.uint8)[:, :, :3]
        if normal.shape[:2] != (height, width):
            raise ValueError(f"{path}: the normal map is {normal.shape[1]}x{normal.shape[0]}, the picture {width}x{height}")
        return normal

    def __getitem__(self, idx):
        image, q, t, info = self.load_raw(idx)
        image = image.permute(2, 0, 1).to(torch.float32).div(255)               # torchvision's to_tensor
        image = image[:3, :info.camera_height, :info.camera_width].contiguous()
        image, info = ImagePoseDataset._autoscale_image_and_camera_info(image, info)
        return image, q, t, info

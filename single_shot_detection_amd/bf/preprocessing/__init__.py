"""bf/preprocessing on the device: the reference's augmentation pipeline as two libssdk calls per batch (csrc/augment.hip)."""
from .device_augmentation import AugmentParams, DeviceAugmentation, IMAGE_DTYPE, PARAMS_DTYPE  # noqa: F401
from .device_augmentation import HUE_SATURATION, BRIGHTNESS, CONTRAST, EXPAND, CROP, HFLIP, VFLIP, KEEP_IOU  # noqa: F401

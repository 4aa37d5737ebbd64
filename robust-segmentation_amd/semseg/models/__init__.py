from .convnext_upernet import CONVNEXT_SETTINGS, ConvNeXt, UperNetForSemanticSegmentation  # noqa: F401
from .deeplabv3 import DeepLabV3  # noqa: F401
from .pspnet import PSPNet  # noqa: F401
from .segmenter import MaskTransformer, SegMenter, VisionTransformer, create_segmenter  # noqa: F401

__all__ = ["UperNetForSemanticSegmentation", "ConvNeXt", "CONVNEXT_SETTINGS", "SegMenter", "VisionTransformer",
           "MaskTransformer", "create_segmenter", "PSPNet", "DeepLabV3"]

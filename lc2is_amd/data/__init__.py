"""Device-side data path in front of the hot path: the reference's CLIPFeatureExtractor image / label
transforms (evaluate.py:58-61, data/collator.py:82-91), the ADE20K collate (data/collator.py:168-180) and the train-time
augmentation the reference reserves a hook for (data/dataset.py:144-149), with the mixed-sample step (ClassMix / CutMix) and the
strong photometric views (colour jitter, greyscale, Gaussian blur) and the geometric views (random affine warp, the labels follow) of
self-training behind it."""
from .augment import AugmentedBatches, DeviceImagePool, TrainAugment, class_weights
from .geo import GeometricAugment
from .mix import SampleMix
from .strong import StrongAugment
from .preprocess import ADE20KCollator, ClipImagePreprocessor, ClipLabelPreprocessor

__all__ = ["ADE20KCollator", "ClipImagePreprocessor", "ClipLabelPreprocessor", "DeviceImagePool", "TrainAugment",
           "AugmentedBatches", "class_weights", "SampleMix", "StrongAugment", "GeometricAugment"]

from .datasets import (CIFAR10, CUB200, DatasetCollection, ImageFolder, Places365Small, SyntheticImages,
                       prepare_dataloaders)
from .gpu_augment import AugmentPlanner, gpu_augment
from . import transforms

__all__ = ["AugmentPlanner", "CIFAR10", "CUB200", "DatasetCollection", "ImageFolder", "Places365Small",
           "SyntheticImages", "gpu_augment", "prepare_dataloaders", "transforms"]

from .datasets import (CIFAR10, CUB200, DatasetCollection, ImageFolder, Places365Small, SyntheticImages,
                       prepare_dataloaders)
from .gpu_augment import AugmentPlanner, gpu_augment
from .rand_augment import RandAugmentPlanner, parse_rand_augment, rand_augment_bytes
from .random_erase import RandomErasePlanner, random_erase_
from . import transforms

__all__ = ["AugmentPlanner", "CIFAR10", "CUB200", "DatasetCollection", "ImageFolder", "Places365Small",
           "RandAugmentPlanner", "RandomErasePlanner", "SyntheticImages", "gpu_augment", "parse_rand_augment",
           "prepare_dataloaders", "rand_augment_bytes", "random_erase_", "transforms"]

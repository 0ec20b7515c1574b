"""dataset_def.py surface for Health-MNIST (reference dataset_def.py:133-219) and Physionet (dataset_def.py:8-44):
the datasets are preloaded into device tensors (lvae_amd.data)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lvae_amd.data import (DeviceBatchLoader, HealthMNISTDataset, HealthMNISTDatasetConv,  # noqa: E402,F401
                           PhysionetDataset)

__all__ = ["HealthMNISTDatasetConv", "HealthMNISTDataset", "PhysionetDataset", "DeviceBatchLoader"]

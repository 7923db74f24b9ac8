from deepfm_amd.data.device_epoch import (BucketDifference, DeviceColumns, DeviceEpochLoader, ItemTable,  # noqa: F401
                                          NegativeSampler, Role, SeenSets)

from deepfm_amd.data.device_epoch import (BucketDifference, CandidateSource, DeviceColumns, DeviceEpochLoader,  # noqa: F401
                                          ItemTable, NegativeSampler, Role, SeenSets, resolve_roles)
from deepfm_amd.data.candidates import CatalogueCandidates, WeightedNegatives, item_weights  # noqa: F401
from deepfm_amd.data.encoders import (DeviceFeatureEncoder, DeviceLabelEncoder, DeviceMinMaxScaler,  # noqa: F401
                                      DeviceMultiHotEncoder)
from deepfm_amd.data.interactions import (DeviceHistoryIndex, DeviceInteractionLog, DeviceSeenSets,  # noqa: F401
                                          HistoryBag, InteractionSplit, UserHistory, count_feature_table,
                                          history_field, popularity_weights)

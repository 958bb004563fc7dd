"""MI355X-native FastSpeech2-with-emotion-intensity train path (drop-in for
Orca0917/fine-grained-emotional-control-of-tts ``emo_rank_tts/fastspeech2``).

    from fastspeech2.model import FastSpeech2      # model.py:32  (same kwargs, 8-tuple)
    from fastspeech2.loss import Loss              # loss.py:6    (same dict of 7 losses)
    from fastspeech2.train import train_step, FusedTrainer
    from fastspeech2.optim import FusedAdamW

The rank model's data path (``emo_rank_tts/rank_model/dataset.py``):

    from fastspeech2 import FineGrainedDataset, RankGpuCollate, RankDeviceStore

The FastSpeech2 data path with the set resident on the device (index-list batches, cached
intensity input):

    from fastspeech2 import FS2DeviceStore
    from fastspeech2.train import train_one_epoch

The log-mel front end (``emo_rank_tts/rank_model/audio_util.py::get_mel``), batched on the GPU:

    from fastspeech2 import MelFrontEnd, get_mel

The prosody feature stage (``emo_rank_tts/rank_model/preprocess.py::feature_extraction``,
:104-168): tracks, outlier-free statistics and finished items from the front end's output:

    from fastspeech2 import ProsodyStage, extract_features, FeatureSet

Compute runs only through libfs2_hip.so (include/fs2_hip.h); see DESIGN.md.
"""

import os

import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))

_RANK_DATASET = ("FineGrainedDataset", "RankGpuCollate", "RankDeviceStore")
_AUDIO = ("MelFrontEnd", "get_mel")
_PROSODY = ("ProsodyStage", "extract_features", "FeatureSet")
__all__ = ["load_config", *_RANK_DATASET, "FS2DeviceStore", *_AUDIO, *_PROSODY]


def __getattr__(name):
    # resolved on first use, so that importing the package alone does not import torch
    if name in _RANK_DATASET:
        from . import rank_dataset
        return getattr(rank_dataset, name)
    if name == "FS2DeviceStore":
        from . import device_store
        return device_store.FS2DeviceStore
    if name in _AUDIO:
        from . import audio
        return getattr(audio, name)
    if name in _PROSODY:
        from . import prosody
        return getattr(prosody, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def load_config(path=None):
    """parameter.yaml with the reference's key names (fastspeech2/parameter.yaml)."""
    with open(path or os.path.join(_HERE, "parameter.yaml")) as f:
        return yaml.safe_load(f)

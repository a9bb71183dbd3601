"""Reference-shaped import path: ``import model.unets as unets; import model.losses as losses`` (as in the
reference's train_model.py:19-22, ``model.augmentations``, ``model.data_generators``, ``model.preprocess``, ``model.detection``, ``model.surface_distance``, ``model.calibration``, ``model.bootstrap``, ``model.validation`` and ``model.tiling`` included) resolves to the MI355X-native package ``prostatemr_3d-cad-cspca_amd``."""
import importlib
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _root not in sys.path:
    sys.path.insert(0, _root)
_pkg = importlib.import_module("prostatemr_3d-cad-cspca_amd")
unets = _pkg.unets
losses = _pkg.losses
initializers = _pkg.initializers
optim = _pkg.optim
augmentations = _pkg.augmentations
data_generators = _pkg.data_generators
preprocess = _pkg.preprocess
detection = _pkg.detection
surface_distance = _pkg.surface_distance
calibration = _pkg.calibration
bootstrap = _pkg.bootstrap
validation = _pkg.validation
tiling = _pkg.tiling
sys.modules[__name__ + ".unets"] = unets
sys.modules[__name__ + ".unets.networks"] = unets.networks
sys.modules[__name__ + ".unets.network_blocks"] = unets.network_blocks
sys.modules[__name__ + ".unets.modelio"] = unets.modelio
sys.modules[__name__ + ".losses"] = losses
sys.modules[__name__ + ".augmentations"] = augmentations
sys.modules[__name__ + ".data_generators"] = data_generators
sys.modules[__name__ + ".preprocess"] = preprocess
sys.modules[__name__ + ".detection"] = detection
sys.modules[__name__ + ".surface_distance"] = surface_distance
sys.modules[__name__ + ".calibration"] = calibration
sys.modules[__name__ + ".bootstrap"] = bootstrap
sys.modules[__name__ + ".validation"] = validation
sys.modules[__name__ + ".tiling"] = tiling

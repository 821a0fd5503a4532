"""Rendering of scored frames (include/pasco_view.h): grid passes, colour-index grids per view, a ray caster and the two
commands around them.  `host` is the numpy restatement of every kernel, `lib` the binding of the `pv_*` entry points,
`frames` turns a saved frame into images on either, `outputs` writes the frames `eval.kitti --save-outputs` saves."""
from . import host  # noqa: F401
from .camera import PRESETS, camera, preset  # noqa: F401
from .frames import VIEW_NAMES, DeviceOps, HostOps, frame_images  # noqa: F401
from .outputs import KEYS, frame_record, save_step_outputs, write_record  # noqa: F401
from .palette import label_palette, ramp_palette  # noqa: F401
from .png import decode_png, encode_png, write_png  # noqa: F401

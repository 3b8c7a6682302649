"""VideoPrism video encoder on AMD MI355X (gfx950).

Drop-in for the reference package `videoprism` (tmoroney/videoprism-mlx): the modules
`models`, `models_mlx`, `utils`, `video_utils` keep the reference's names and signatures; the
forward pass and the frame preprocessing run in hand-written HIP kernels (libvideoprism_hip.so,
C-ABI in include/videoprism_hip.h) loaded through `videoprism._native`.
"""

__version__ = "0.1.0"

from . import video_utils  # noqa: E402,F401
from .video_utils import load_video, load_video_batch, preprocess_frames, preprocess_yuv_frames  # noqa: E402,F401

"""Plugin registry mirroring /root/reference/models/__init__.py:1-7: the CLIs resolve detector,
encoder and classifier classes with getattr(models, <name>)(**json_kwargs)
(demo_image.py:361-374,378-382, demo_video.py:260-273, find_embedding.py:77)."""
from .encoders import InceptionResnetV1, iresnet100, resnet101  # noqa: F401
from .classifier import MLPModel  # noqa: F401
from .gallery import GalleryModel  # noqa: F401
from .detector import MTCNN  # noqa: F401
from .retina import RetinaFace  # noqa: F401
from .emotion import resnet_2branch_50  # noqa: F401


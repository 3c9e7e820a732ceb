from .coco_evaluation import coco_average_precision, coco_evaluation  # noqa: F401

"""Install the MI355X path behind the reference's plugin surface."""
import sys


def install_pointops():
    """Make ``import pointops`` (libs/pointops/functions/__init__.py:1-14 names) and ``import pointops2.pointops``
    (the window-attention part, libs/pointops2/functions/pointops.py) and ``import pointgroup_ops`` (libs/pointgroup_ops:
    ``ballquery_batch_p``, ``bfs_cluster``) resolve to this package's drop-ins."""
    from . import pointgroup_ops, pointops, pointops2

    sys.modules["pointops"] = pointops
    # libs/pointops2: ``import pointops2.pointops as pointops`` (stratified_transformer_v1m1_origin.py:21)
    sys.modules["pointops2"] = pointops2
    sys.modules["pointops2.pointops"] = pointops2.pointops
    sys.modules["pointgroup_ops"] = pointgroup_ops
    return pointops


def register_into_pointcept(force=True):
    """Register our classes under the reference's names in a live pointcept install's registries."""
    from pointcept.models.builder import MODELS as PC_MODELS  # noqa: import error = pointcept not importable
    from . import cac, masked_scene_contrast, point_group, point_transformer, point_transformer_v2, point_transformer_v3, recognizer, segmentor, model_hook, sparse_unet, stratified  # noqa: F401  (fills the registries)
    from .registry import MODELS, RECOGNIZER, MODELHOOKS

    for name in ["PointTransformer-Seg26", "PointTransformer-Seg38", "PointTransformer-Seg50",
                 "PointTransformer-Recognizer", "ST-v1m1", "ST-v1m1-Recognizer", "PT-v2m2", "DefaultSegmentor", "CAC-v1m1", "SpUNet-v1m1", "PT-v3m1", "DefaultSegmentorV2", "PG-v1m1", "MSC-v1m1"]:
        PC_MODELS.register_module(name=name, force=force, module=MODELS.get(name))
    try:
        from pointcept.recognizers.builder import RECOGNIZER as PC_REC

        for name in ["PointPdf-v1m1", "MaxProbability"]:
            PC_REC.register_module(name=name, force=force, module=RECOGNIZER.get(name))
    except ImportError:
        pass
    try:
        from pointcept.incrLearners.builder import INCREMENTALLEARNER as PC_INCR
        from . import incremental  # noqa: F401  (fills the registry)
        from .registry import INCREMENTALLEARNER

        PC_INCR.register_module(name="PointPdf-incr-v1m1", force=force, module=INCREMENTALLEARNER.get("PointPdf-incr-v1m1"))
    except ImportError:
        pass
    try:
        from pointcept.models.utils.model_hook import MODELHOOKS as PC_HOOKS

        PC_HOOKS.register_module(name="ModelHook", force=force, module=MODELHOOKS.get("ModelHook"))
    except ImportError:
        pass


def register_losses_into_pointcept(force=True):
    """Register ``LovaszLoss`` (losses.py: the capturable HIP pass on the device) under the reference's name in a live pointcept
    install's ``pointcept.models.losses.builder.LOSSES``, so that its own ``build_criteria`` builds ours."""
    from pointcept.models.losses.builder import LOSSES as PC_LOSSES  # noqa: import error = pointcept not importable
    from . import losses  # noqa: F401  (fills the registry)
    from .registry import LOSSES

    PC_LOSSES.register_module(name="LovaszLoss", force=force, module=LOSSES.get("LovaszLoss"))


def register_criteria_into_pointcept(force=True, cross_entropy=True):
    """The criteria of the reference's losses/misc.py likewise: ``FocalLoss``, ``DiceLoss``, ``BinaryFocalLoss`` (losses.py) and, unless
    ``cross_entropy=False``, ``CrossEntropyLoss`` (segmentor.py: class weights, label smoothing, every reduction and any class count as
    capturable HIP passes; the reference's own class stays usable, through torch's kernels)."""
    from pointcept.models.losses.builder import LOSSES as PC_LOSSES  # noqa: import error = pointcept not importable
    from . import losses, segmentor  # noqa: F401  (fill the registry)
    from .registry import LOSSES

    for name in ["FocalLoss", "DiceLoss", "BinaryFocalLoss"] + (["CrossEntropyLoss"] if cross_entropy else []):
        PC_LOSSES.register_module(name=name, force=force, module=LOSSES.get(name))

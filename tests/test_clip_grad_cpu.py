"""clip_grad plumbing that needs no GPU: the command line, the step configuration's default and the parameter
layout that lets to_rgb_8 train."""
import pytest


def test_train_model_parser_clip_grad():
    import train_model
    args = train_model.parse_args(["--clip_weights", "clip.pt", "--clip_grad"])
    assert args.clip_grad is True and args.clip_weights == "clip.pt"
    assert train_model.parse_args([]).clip_grad is False
    with pytest.raises(SystemExit):
        train_model.parse_args(["--clip_grad"])  # the tower whose backward it runs comes from --clip_weights


def test_step_config_default_is_off():
    from moegan_mi.step import StepConfig
    assert StepConfig().clip_grad is False
    assert StepConfig(clip_grad=True).clip_grad is True


def test_frozen_prefixes_follow_clip_grad():
    from moegan_mi.layout import frozen_rgb_prefixes
    assert frozen_rgb_prefixes(16) == ("to_rgb_8.",)  # the reference
    assert frozen_rgb_prefixes(16, clip_grad=True) == ()
    assert frozen_rgb_prefixes(64, clip_grad=True) == frozen_rgb_prefixes(64)[:-1]  # the half-resolution layer trains


def test_flat_order_puts_to_rgb_8_in_the_optimised_range():
    from moegan_mi.layout import frozen_rgb_prefixes, generator_shapes
    from moegan_mi.params import ParamStore, flat_order
    shapes = generator_shapes(4)
    order, frozen = flat_order(shapes, frozen_rgb_prefixes(16, clip_grad=True))
    assert not frozen and all(n in order for n in shapes if n.startswith("to_rgb_8."))
    order_ref, frozen_ref = flat_order(shapes, frozen_rgb_prefixes(16))
    assert all(n.startswith("to_rgb_8.") for n in frozen_ref) and len(frozen_ref) == 3
    st = ParamStore(shapes, "cpu", frozen_prefixes=())
    off, _ = st.offsets["to_rgb_8.weight"]
    assert off < st.n_main <= st.n_opt  # inside the main optimizer launch's range
    assert st.offsets["to_rgb_8.modulation.weight"][0] < st.n_main  # (its style rides the batched style GEMM)


def test_foreign_encoder_detection():
    from moegan_mi.step import clip_tower

    class Tower:
        def encode_image(self, im):
            return im

        def encode_generated(self, im, save=False):
            return im

        def backward(self, *a, **k):
            pass
    t = Tower()
    assert clip_tower(t) is t and clip_tower(t.encode_image) is t
    assert clip_tower(lambda im: im) is None

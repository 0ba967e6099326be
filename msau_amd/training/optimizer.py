"""`get_optimizer` counterpart (reference: model/training/optimizer.py:4-31).

Table-driven: the option names and their defaults are the reference's -- `optimizer` in {"momentum", "rmsprop"
(default), anything else = Adam}, `learning_rate` 1e-3, `momentum` 0.9 -- and so is its quirk of handing
`lr_decay_rate` to the optimizer as *weight decay*.  Prints the same two lines the reference prints."""
import torch

_DEFAULTS = {"optimizer": "rmsprop", "learning_rate": 1e-3, "lr_decay_rate": 0.0, "momentum": 0.9}


def _adam(parameters, opt):
    if opt["learning_rate"] is None:                 # the reference then falls back to torch's own defaults
        return torch.optim.Adam(parameters)
    return torch.optim.Adam(parameters, lr=opt["learning_rate"], weight_decay=opt["lr_decay_rate"])


_FACTORIES = {
    "momentum": lambda parameters, opt: torch.optim.SGD(parameters, lr=opt["learning_rate"], momentum=opt["momentum"],
                                                        weight_decay=opt["lr_decay_rate"]),
    "rmsprop": lambda parameters, opt: torch.optim.RMSprop(parameters, lr=opt["learning_rate"],
                                                           weight_decay=opt["lr_decay_rate"]),
}


def get_optimizer(model, kwargs={}):
    opt = {key: kwargs.get(key, default) for key, default in _DEFAULTS.items()}
    made = _FACTORIES.get(opt["optimizer"], _adam)(model.parameters(), opt)
    shown = "" if opt["learning_rate"] is None else str(opt["learning_rate"])
    print(f"Optimizer: {opt['optimizer']}")
    print(f"Learning Rate: {shown}")
    return made


def engine_options(kwargs={}) -> dict:
    """`get_optimizer`'s options as keyword arguments of `msau_amd.TrainEngine` (the device path's optimiser, `TrainEngine.
    from_opt_kwargs`): the same table -- "momentum" = SGD with momentum, "rmsprop" (default), any other name Adam; `learning_rate`
    1e-3, None = Adam with torch's own defaults (the other two need a rate, as torch does); `lr_decay_rate` as weight decay --
    and `max_norm=None`, because the reference's `Trainer.train` never clips.  "shown": the two values `get_optimizer` prints."""
    opt = {key: kwargs.get(key, default) for key, default in _DEFAULTS.items()}
    kind = opt["optimizer"] if opt["optimizer"] in _FACTORIES else "adam"
    shown = (opt["optimizer"], "" if opt["learning_rate"] is None else str(opt["learning_rate"]))
    if opt["learning_rate"] is None:
        if kind != "adam":
            raise ValueError(f"optimizer {kind!r} needs a learning_rate")
        return {"optimizer": "adam", "lr": 1e-3, "weight_decay": 0.0, "max_norm": None, "shown": shown}       # torch.optim.Adam()
    out = {"optimizer": kind, "lr": float(opt["learning_rate"]), "weight_decay": float(opt["lr_decay_rate"]), "max_norm": None,
           "shown": shown}
    if kind == "momentum":
        out["momentum"] = float(opt["momentum"])
    return out

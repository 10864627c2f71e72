"""Drop-in for the reference's utils/early_stopping.py::EarlyStopping, with its rule kept as written:

  * every call counts one epoch; a score <= the best so far (>= with low_is_good=False) is a new best -- an EQUAL score too -- and stores
    a deep copy of the model's state_dict (:49-53, :66-69, :92);
  * otherwise `epoch > best_epoch + patience` returns True (:54-56), else False;
  * `best_state` loads the stored weights back into the model it was built with and returns that model (:71-85).

The reference writes the state to "<path_prefix>_<model_name>.pkl" at every new best and again at every restore.  Here the copy is held
in memory and a file is written only when a path_prefix is given (the reference's own loops pass "").  After a restore the parameters
have changed under the engine's cached low-precision weight operands, so they are invalidated the way utils.global_functions.load_model
does (engine.bump_weight_epoch)."""
from copy import deepcopy

import torch


class EarlyStopping:
    def __init__(self, path_prefix, model, patience=8, low_is_good=True, hyperopt=False, verbose=False, model_name=""):
        self.patience = patience
        self.best_score = None
        self.best_epoch = 0
        self.epoch = 0
        self.low_is_good = low_is_good
        self.path_prefix = f"{path_prefix}_{model_name}.pkl" if path_prefix else None
        self.hyperopt = hyperopt
        self.verbose = verbose
        self.model = model
        self.best_state_dict = None

    def __call__(self, model, score):
        """One epoch's score -> True when training has gone `patience` epochs past the best one."""
        self.epoch += 1
        if self.best_score is None:
            self.best_score = score
        if self.new_best(score):
            self.best_state = model
            self.best_score = score
            self.best_epoch = self.epoch
            return False
        elif self.epoch > self.best_epoch + self.patience:
            print("Early stopping: Terminate", flush=True)
            return True
        if self.verbose:
            print("Early stopping: Worse epoch", flush=True)
        return False

    def new_best(self, score):
        return score <= self.best_score if self.low_is_good else score >= self.best_score

    @property
    def best_state(self):
        """Load the best weights back into the model and return it."""
        if self.best_state_dict is None:
            raise RuntimeError("EarlyStopping.best_state: no state has been stored yet")
        print(f"Loading weights from epoch {self.best_epoch}", flush=True)
        self.model.load_state_dict(self.best_state_dict["model_state_dict"])
        from .. import engine
        engine.bump_weight_epoch()               # parameters changed: cached low-precision operand copies must refresh
        if self.path_prefix is not None:
            torch.save({"model_state_dict": self.best_state_dict}, self.path_prefix)
        return self.model

    @best_state.setter
    def best_state(self, model):
        self.best_state_dict = deepcopy({"model_state_dict": model.state_dict()})
        if self.path_prefix is not None:
            torch.save({"model_state_dict": model.state_dict()}, self.path_prefix)

"""What models/BooleanModel.py gives the seven combinatorial models, held on every one of them without a GPU: the refusals, the scores
from the engine's counts and their cache, and that no model keeps a copy of its own.  The engines are the NumPy stand-ins of the
models' own CPU tests; the fits against the recorded reference results are in those tests.  Also the packed-word helpers of
pybmf_amd/bitset.py.
"""
import contextlib
import io

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import grecondplus_ref as GP
import test_asso_cpu as A
import test_asso_refine_cpu as AR
import test_grecond_cpu as G
import test_mebf_cpu as ME
import test_panda_cpu as P

FIT_KW = G.FIT_KW
SHARED = ("_counts_of", "_score", "_make_X_pd", "_init_factors")

X = np.zeros((12, 10))
X[:6, :5] = X[6:, 5:] = 1
X[0, 9] = 1
U0, V0 = np.zeros((12, 2)), np.zeros((10, 2))
U0[:6, 0] = U0[6:, 1] = V0[:5, 0] = V0[5:, 1] = 1

# class name -> (constructor keywords, the stand-in engine of the model's own CPU test)
MODELS = {
    "GreConD": (lambda: dict(k=2), G.numpy_engine),
    "GreConDPlus": (lambda: dict(k=2), GP.numpy_engine),
    "Asso": (lambda: dict(tau=0.5, k=2), A.numpy_engine),
    "AssoIter": (lambda: dict(model=AR.stand_in_model(U0, V0)), AR.numpy_engine),
    "AssoOpt": (lambda: dict(model=AR.stand_in_model(U0, V0)), AR.numpy_engine),
    "MEBF": (lambda: dict(k=2, t=0.5), ME.numpy_engine),
    "Panda": (lambda: dict(k=2), P.numpy_engine),
}


def fitted(name, X_val=None):
    """The real class on X with its stand-in engine; model._asked lists the data sets the engine was asked to count."""
    import pybmf_amd.models as M
    params, factory = MODELS[name]

    class Model(getattr(M, name)):
        def _make_engine(self):
            eng, self._asked = factory(self), []
            counts = eng.counts

            def counted(name="train"):
                self._asked.append(name)
                return counts(name)
            eng.counts = counted
            return eng
    model = Model(**params())
    model.fit(csr_matrix(X), None if X_val is None else csr_matrix(X_val), **FIT_KW)
    return model


@pytest.mark.parametrize("name", list(MODELS))
def test_what_the_base_class_owns(name):
    import pybmf_amd.models as M
    cls, params = getattr(M, name), MODELS[name][0]
    assert issubclass(cls, M.BooleanModel) and not any(attr in cls.__dict__ for attr in SHARED)
    with contextlib.redirect_stdout(io.StringIO()):
        # refused before an engine is made: these run the class as it is, device engine and all
        with pytest.raises(NotImplementedError, match="reconstruction"):
            cls(**params()).fit(csr_matrix(X), **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            cls(**params()).fit(X * 3, **FIT_KW)
        with pytest.raises(NotImplementedError, match="Boolean"):
            cls(**params()).fit(csr_matrix(X), csr_matrix(X * 3), **FIT_KW)
        model = fitted(name)
        with pytest.raises(NotImplementedError, match="Boolean metrics"):
            model._score("train", ["Recall", "RMSE"])
        with pytest.raises(ValueError, match="no val data"):
            model._score("val", ["Recall"])
        model = fitted(name, X_val=X)
    # one question per data set between two _invalidate() calls, whoever asks
    for _ in range(2):
        model._invalidate()
        del model._asked[:]
        assert model.X_pd is not None             # (rebuilt from the engine's bits; no count is asked for)
        first = [model._counts_of("train"), model._counts_of("val")]
        model._score("val", ["Recall", "F1"])
        model._train_error()
        assert [model._counts_of("train"), model._counts_of("val")] == first and model._asked == ["train", "val"]
    tp, fp, fn, tn = first[0]
    assert tp + fp + fn + tn == X.size and tp + fn == int(X.sum())
    assert model._train_error() == 1 - np.float64(tp + tn) / X.size


@pytest.mark.parametrize("length", [1, 31, 32, 33, 2049])
def test_pack_bits_round_trip(length):
    from pybmf_amd.bitset import bit_positions, pack_bits, popcount, unpack_bits
    rng = np.random.RandomState(length)
    words = -(-length // 32) + 1
    for flags in (rng.rand(length) < 0.4, np.ones(length, dtype=bool), np.zeros(length, dtype=bool)):
        w = pack_bits(flags, words)
        assert w.dtype == np.uint32 and w.shape == (words,)
        assert unpack_bits(w, length).tolist() == flags.tolist() and not unpack_bits(w, words * 32)[length:].any()
        assert popcount(w) == int(flags.sum()) and bit_positions(w).tolist() == np.nonzero(flags)[0].tolist()

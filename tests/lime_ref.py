"""numpy + scikit-learn restatement of lime 0.2.0.1's ``LimeImageExplainer.explain_instance`` (lime_image.py, lime_base.py) and of
``ImageExplanation.get_image_and_mask``, taking any ``classifier_fn`` -- the reference the LIME tests compare brainxai.lime_image
with.  The package itself is not a dependency; where ``import lime`` succeeds one test compares the two."""
from types import SimpleNamespace

import numpy as np
from sklearn.linear_model import Ridge
from sklearn.metrics import pairwise_distances


def draw_masks(num_samples, n_features, random_state):
    """lime_image.data_labels: one randint call per image on the explainer's RandomState, row 0 all ones."""
    data = random_state.randint(0, 2, num_samples * n_features).reshape((num_samples, n_features))
    data[0, :] = 1
    return data


def fudged_image(image, segments, hide_color=None):
    fudged = image.copy()
    if hide_color is None:
        for x in np.unique(segments):
            fudged[segments == x] = tuple(np.mean(image[segments == x][:, c]) for c in range(image.shape[2]))
    else:
        fudged[:] = hide_color
    return fudged


def perturbed_images(image, segments, fudged, data):
    """The neighbourhood as the package builds it (same dtype as the image)."""
    out = []
    for row in data:
        temp = image.copy()
        mask = np.zeros(segments.shape, dtype=bool)
        for z in np.where(row == 0)[0]:
            mask[segments == z] = True
        temp[mask] = fudged[mask]
        out.append(temp)
    return out


def distances(data):
    return pairwise_distances(data, data[0].reshape(1, -1), metric="cosine").ravel()


def distances_closed_form(data):
    """row 0 is all ones: d_n = 1 - sqrt(sum_s z_ns / S) (an all-zero row: 1, as scikit-learn's normalisation gives)"""
    return 1.0 - np.sqrt(data.sum(1) / data.shape[1])


def kernel(d, kernel_width=0.25):
    return np.sqrt(np.exp(-(d ** 2) / kernel_width ** 2))


def ridge_closed_form(X, y, w, alpha):
    """Ridge(alpha, fit_intercept=True).fit(X, y, sample_weight=w): (coef, intercept, score, prediction for row 0)."""
    X, y, w = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(w, np.float64)
    W = w.sum()
    xb, yb = (w[:, None] * X).sum(0) / W, (w * y).sum() / W
    Xc, yc = X - xb, y - yb
    A = Xc.T @ (w[:, None] * Xc) + alpha * np.eye(X.shape[1])
    beta = np.linalg.solve(A, Xc.T @ (w * yc))
    icpt = yb - xb @ beta
    pred = X @ beta + icpt
    score = 1.0 - (w * (y - pred) ** 2).sum() / (w * (y - yb) ** 2).sum()
    return beta, icpt, score, pred[0]


def ridge_system(X, w, alpha):
    """The matrix of the normal equations (for its condition number)."""
    X, w = np.asarray(X, np.float64), np.asarray(w, np.float64)
    Xc = X - (w[:, None] * X).sum(0) / w.sum()
    return Xc.T @ (w[:, None] * Xc) + alpha * np.eye(X.shape[1])


def ridge_sklearn(X, y, w, alpha):
    m = Ridge(alpha=alpha, fit_intercept=True).fit(X, y, sample_weight=w)
    return m.coef_, float(m.intercept_), float(m.score(X, y, sample_weight=w)), float(m.predict(X[0].reshape(1, -1))[0])


def select_features(data, y, w, num_features, method):
    if method == "auto":
        method = "forward_selection" if num_features <= 6 else "highest_weights"
    if method == "none":
        return np.arange(data.shape[1])
    if method == "highest_weights":
        coef = Ridge(alpha=0.01, fit_intercept=True).fit(data, y, sample_weight=w).coef_
        weighted = coef * data[0]
        ranked = sorted(zip(range(data.shape[1]), weighted), key=lambda x: np.abs(x[1]), reverse=True)
        return np.array([x[0] for x in ranked[:num_features]])
    raise ValueError(method)


def explain(image, segments, classifier_fn, labels=None, top_labels=5, hide_color=None, num_features=100000, num_samples=1000,
            feature_selection="auto", kernel_width=0.25, alpha=1.0, seed=0, random_state=None, masks=None):
    """Steps 1-7.  Returns a namespace with the package's attributes plus masks, probs, weights, used {label: features}."""
    rs = random_state if random_state is not None else np.random.RandomState(seed)
    S = np.unique(segments).shape[0]
    data = draw_masks(num_samples, S, rs) if masks is None else np.asarray(masks).astype(np.int64)
    data[0, :] = 1
    fudged = fudged_image(image, segments, hide_color)
    probs = np.asarray(classifier_fn(np.array(perturbed_images(image, segments, fudged, data))))
    w = kernel(distances(data), kernel_width)
    e = SimpleNamespace(image=image, segments=segments, masks=data, probs=probs, weights=w, local_exp={}, intercept={}, score={},
                        local_pred={}, used={}, top_labels=None)
    if labels is None:
        e.top_labels = [int(k) for k in np.argsort(probs[0])[-top_labels:]][::-1]
        labels = e.top_labels
    for k in labels:
        y = probs[:, k]
        used = select_features(data, y, w, num_features, feature_selection)
        coef, icpt, score, pred = ridge_sklearn(data[:, used], y, w, alpha)
        e.used[k] = used
        e.local_exp[k] = sorted(zip((int(f) for f in used), (float(c) for c in coef)), key=lambda x: np.abs(x[1]), reverse=True)
        e.intercept[k], e.score[k], e.local_pred[k] = icpt, score, pred
    return e


def get_image_and_mask(e, label, positive_only=True, negative_only=False, hide_rest=False, num_features=5, min_weight=0.0):
    """ImageExplanation.get_image_and_mask of lime 0.2.0.1 on a namespace with image, segments, local_exp."""
    if label not in e.local_exp:
        raise KeyError("Label not in explanation")
    if positive_only & negative_only:
        raise ValueError("Positive_only and negative_only cannot be true at the same time.")
    segments, image, exp = e.segments, e.image, e.local_exp[label]
    mask = np.zeros(segments.shape, segments.dtype)
    temp = np.zeros(image.shape) if hide_rest else image.copy()
    if positive_only:
        fs = [x[0] for x in exp if x[1] > 0 and x[1] > min_weight][:num_features]
    if negative_only:
        fs = [x[0] for x in exp if x[1] < 0 and abs(x[1]) > min_weight][:num_features]
    if positive_only or negative_only:
        for f in fs:
            temp[segments == f] = image[segments == f].copy()
            mask[segments == f] = 1
        return temp, mask
    for f, w in exp[:num_features]:
        if np.abs(w) < min_weight:
            continue
        c = 0 if w < 0 else 1
        mask[segments == f] = -1 if w < 0 else 1
        temp[segments == f] = image[segments == f].copy()
        temp[segments == f, c] = np.max(image)
    return temp, mask

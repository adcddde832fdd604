"""fp64 restatement of the shaped losses: TF 1.15's tf.losses.mean_squared_error / huber_loss / softmax_cross_entropy with
``weights=`` (one per sample), ``label_smoothing=`` and ``delta=``, reduction SUM_BY_NONZERO_WEIGHTS.  Written from the formulas; imports
nothing from geeco_amd.  torch autograd differentiates it."""
import torch

MSE, XENT, HUBER = 0, 1, 2


def _f64(t):
  return t if torch.is_tensor(t) and t.dtype == torch.float64 else torch.as_tensor(t, dtype=torch.float64)


def nonzero_mean(per_sample, weights, size):
  """sum_n w_n per_sample_n / (size * #{n: w_n != 0}); 0 when no weight is non-zero (TF's safe division)."""
  count = int((weights != 0).sum())
  if count == 0:
    return (per_sample * 0.0).sum()
  return (weights * per_sample).sum() / (size * count)


def mse_loss(pred, target, weights=None):
  pred, target = _f64(pred), _f64(target)
  w = torch.ones(pred.shape[0], dtype=torch.float64) if weights is None else _f64(weights)
  return nonzero_mean(((pred - target) ** 2).sum(1), w, pred.shape[1])


def huber_loss(pred, target, delta, weights=None):
  """l = 0.5 q^2 + delta (a - q), a = |pred - target|, q = min(a, delta) (TF keeps the factor 0.5 here and not in MSE)."""
  pred, target = _f64(pred), _f64(target)
  w = torch.ones(pred.shape[0], dtype=torch.float64) if weights is None else _f64(weights)
  a = (pred - target).abs()
  q = torch.clamp(a, max=float(delta))
  return nonzero_mean((0.5 * q * q + float(delta) * (a - q)).sum(1), w, pred.shape[1])


def smoothed_one_hot(labels, classes, smoothing=0.0):
  """one_hot(labels) * (1 - smoothing) + smoothing / classes; an out-of-range label keeps an all-zero one-hot."""
  labels = torch.as_tensor(labels).long()
  oh = torch.zeros(labels.shape[0], classes, dtype=torch.float64)
  ok = (labels >= 0) & (labels < classes)
  oh[ok.nonzero()[:, 0], labels[ok]] = 1.0
  return oh * (1.0 - smoothing) + smoothing / classes


def xent_loss(logits, labels, weights=None, smoothing=0.0, class_weights=None):
  """labels: class indices (already rint(target) + 1).  ``class_weights``: the sample weights are multiplied by class_weights[label]
  (0 for an out-of-range label), what a TF user passes as weights=tf.gather(class_weights, labels)."""
  logits = _f64(logits)
  labels = torch.as_tensor(labels).long()
  C = logits.shape[1]
  w = torch.ones(logits.shape[0], dtype=torch.float64) if weights is None else _f64(weights).clone()
  if class_weights is not None:
    cw = _f64(class_weights)
    ok = (labels >= 0) & (labels < C)
    w = w * torch.where(ok, cw[labels.clamp(0, C - 1)], torch.zeros((), dtype=torch.float64))
  y = smoothed_one_hot(labels, C, smoothing)
  per = -(y * torch.log_softmax(logits, dim=1)).sum(1)
  return nonzero_mean(per, w, 1)


def heads_losses(preds, heads, targets, sample_weights=None, class_weights=None, smoothing=0.0, deltas=None):
  """``heads``: [(size, kind, head weight)]; ``preds`` / ``targets``: one [N][size] tensor per head (kind XENT: targets [N][1] hold the
  gripper command, label = rint(target) + 1).  Returns (total, [L_i])."""
  parts = []
  for i, ((size, kind, _), pr, tg) in enumerate(zip(heads, preds, targets)):
    if kind == MSE:
      parts.append(mse_loss(pr, tg, sample_weights))
    elif kind == HUBER:
      parts.append(huber_loss(pr, tg, deltas[i], sample_weights))
    else:
      parts.append(xent_loss(pr, torch.round(_f64(tg)[:, 0]).long() + 1, sample_weights, smoothing, class_weights))
  total = sum(wt * l for (_, _, wt), l in zip(heads, parts))
  return total, parts


def tail_reference(h, w1, b1, hw, hb, heads, targets, **shaping):
  """The decoder tail in fp64 with autograd: a1 = relu(h w1 + b1), pred_i = a1 hw_i + hb_i, the shaped losses.  Returns
  dict(preds=[N][sum sizes], total, parts, grads=dict(h, w1, b1, hw=[...], hb=[...]))."""
  leaves = [t.detach().double().cpu().requires_grad_(True) for t in [h, w1, b1] + list(hw) + list(hb)]
  hd, w1d, b1d = leaves[:3]
  nh = len(heads)
  hwd, hbd = leaves[3:3 + nh], leaves[3 + nh:]
  a1 = torch.relu(hd @ w1d + b1d)
  preds = [a1 @ w_ + b_ for w_, b_ in zip(hwd, hbd)]
  total, parts = heads_losses(preds, heads, [t.detach().double().cpu() for t in targets], **shaping)
  if total.requires_grad:
    total.backward()
  z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
  return dict(preds=torch.cat(preds, 1).detach(), total=total.detach(), parts=torch.stack(parts).detach(),
              grads=dict(h=z(hd), w1=z(w1d), b1=z(b1d), hw=[z(t) for t in hwd], hb=[z(t) for t in hbd]))

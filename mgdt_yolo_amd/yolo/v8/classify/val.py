"""reference: yolo/v8/classify/val.py:10-73 - the classification task's validator.

Per batch one mgdt_cls_topk_fwd launch: the min(nc, 5) best classes of every row (the reference's `argsort(1, descending=True)[:, :n5]`) and the
confusion counts matrix[top1][target] += 1 (ConfusionMatrix.process_cls_preds, metrics.py:197-207) accumulated on the device.  Nothing is read
back until `get_stats`: one host read of the collected rows, the targets and the matrix.  Plots are host tooling outside this package: they
raise."""
import torch

from .... import ops as hip
from ...utils.metrics import ClassifyMetrics

__all__ = ('ClassificationValidator',)


class ClassificationValidator:
    def __init__(self, device='cuda:0', args=None):
        self.device = torch.device(device)
        if (args or {}).get('plots'):
            raise RuntimeError('ClassificationValidator: plots=True is host-side tooling outside the validation path')
        self.metrics = ClassifyMetrics()
        self.names, self.nc = None, None

    def get_desc(self):
        return ('%22s' + '%11s' * 2) % ('classes', 'top1_acc', 'top5_acc')

    def init_metrics(self, names_or_nc):
        """val.py:23-28 with a model's `names` dict (or just the class count)."""
        self.names = dict(names_or_nc) if isinstance(names_or_nc, dict) else {i: f'{i}' for i in range(int(names_or_nc))}
        self.nc = len(self.names)
        if self.nc < 1:
            raise RuntimeError('ClassificationValidator: no classes')
        self.matrix = torch.zeros(self.nc, self.nc, dtype=torch.int32, device=self.device)
        self.pred, self.targets = [], []
        self.confusion_matrix = None

    def preprocess(self, batch):
        """val.py:30-35: image and labels to the device (labels that arrive on the host are range-checked first)."""
        batch = dict(batch)
        cls = batch['cls']
        if torch.is_tensor(cls) and not cls.is_cuda and cls.numel() and (int(cls.min()) < 0 or int(cls.max()) >= self.nc):
            raise ValueError(f'classification label outside [0, {self.nc})')
        batch['img'] = batch['img'].to(self.device, non_blocking=True)
        batch['cls'] = cls.to(self.device).long().reshape(-1)
        return batch

    def update_metrics(self, preds, batch):
        """val.py:37-41: one launch; the rows stay on the device."""
        preds = preds[0] if isinstance(preds, (list, tuple)) else preds
        if preds.shape[1] != self.nc:
            raise RuntimeError(f'ClassificationValidator: the predictions have {preds.shape[1]} classes, the metrics {self.nc}')
        self.pred.append(hip.cls_topk(preds.float(), batch['cls'], self.matrix))
        self.targets.append(batch['cls'])

    def finalize_metrics(self, speed=None):
        """val.py:43-52 without the plots: the confusion counts come to the host."""
        self.confusion_matrix = self.matrix.cpu().numpy()
        if speed is not None:
            self.metrics.speed = speed

    def get_stats(self):
        """val.py:54-57: the one host read, then ClassifyMetrics.process."""
        self.metrics.process([torch.cat(self.targets).cpu()], [torch.cat(self.pred).cpu()])
        return self.metrics.results_dict

    def plot_val_samples(self, batch, ni):
        raise RuntimeError('ClassificationValidator: plots are host-side tooling outside the validation path')

    plot_predictions = plot_val_samples

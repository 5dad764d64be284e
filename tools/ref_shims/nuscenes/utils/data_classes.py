import numpy as np


class LidarPointCloud(object):
    def __init__(self, points):
        assert points.shape[0] == 4
        self.points = points

    @classmethod
    def from_file(cls, file_name):
        assert file_name.endswith('.bin')
        scan = np.fromfile(file_name, dtype=np.float32)
        points = scan.reshape((-1, 5))[:, :4]
        return cls(points.T)

    def nbr_points(self):
        return self.points.shape[1]

    def remove_close(self, radius):
        x_filt = np.abs(self.points[0, :]) < radius
        y_filt = np.abs(self.points[1, :]) < radius
        not_close = np.logical_not(np.logical_and(x_filt, y_filt))
        self.points = self.points[:, not_close]

    def transform(self, transf_matrix):
        self.points[:3, :] = transf_matrix.dot(np.vstack((self.points[:3, :], np.ones(self.nbr_points()))))[:3, :]

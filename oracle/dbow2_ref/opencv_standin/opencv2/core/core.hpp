// TEST INFRASTRUCTURE: stand-in for <opencv2/core/core.hpp>, on the include path of the `dbow2_ref` target of oracle/Makefile only.
// The reference's vendored DBoW2 uses OpenCV for a 1x32 cv::Mat of bytes (FORB::TDescriptor) and for
// cv::FileStorage, which neither loadFromTextFile nor loadFromBinaryFile calls.  This header gives exactly
// that much: a reference-counted byte matrix without arithmetic, and FileStorage / FileNode that only link.
// create() zero-fills; the real cv::Mat::create leaves the bytes indeterminate (DESIGN.md "Oracle").
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

typedef unsigned char uchar;

namespace cv {

class Mat {
public:
    int rows = 0, cols = 0;
    uchar *data = nullptr;
    size_t step = 0;

    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }

    void create(int r, int c, int type)
    {
        const size_t es = elem_size(type);
        if (data && rows == r && cols == c && esz_ == es) return;
        rows = r;
        cols = c;
        esz_ = es;
        step = (size_t)c * es;
        buf_ = std::make_shared<std::vector<uchar> >((size_t)r * step, (uchar)0);
        data = buf_->empty() ? nullptr : buf_->data();
    }
    void release()
    {
        buf_.reset();
        data = nullptr;
        rows = cols = 0;
        step = 0;
    }
    Mat clone() const
    {
        Mat m;
        if (data) {
            m.rows = rows; m.cols = cols; m.esz_ = esz_; m.step = (size_t)cols * esz_;
            m.buf_ = std::make_shared<std::vector<uchar> >((size_t)rows * m.step);
            m.data = m.buf_->data();
            for (int r = 0; r < rows; ++r) memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, m.step);
        }
        return m;
    }
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
    Mat row(int r) const
    {
        Mat m(*this);
        m.rows = 1;
        m.data = data + (size_t)r * step;
        return m;
    }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    template <typename T> T *ptr(int r = 0) { return reinterpret_cast<T *>(data + (size_t)r * step); }
    template <typename T> const T *ptr(int r = 0) const { return reinterpret_cast<const T *>(data + (size_t)r * step); }
    template <typename T> T &at(int r, int c) { return ptr<T>(r)[c]; }
    template <typename T> const T &at(int r, int c) const { return ptr<T>(r)[c]; }

private:
    static size_t elem_size(int type) { return type == CV_32F ? 4 : 1; }
    size_t esz_ = 1;
    std::shared_ptr<std::vector<uchar> > buf_;
};

// The YAML path (save / load through cv::FileStorage) is virtual in TemplatedVocabulary and therefore
// instantiated; nothing calls it.  isOpened() is false, so the reference's own callers would throw.
class FileNode {
public:
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    operator int() const { return 0; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
    size_t size() const { return 0; }
    int type() const { return 0; }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const std::string &, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](const char *) const { return FileNode(); }
};

template <typename T> inline FileStorage &operator<<(FileStorage &fs, const T &) { return fs; }

}  // namespace cv
